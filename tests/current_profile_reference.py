"""The sheared current of hydro_step_fused_tiled_multi_shear (include/hydro.h, "Current profile") for tests/test_current_profile.py
and tests/test_current_profile_gpu.py: the "shear" row of the resident harness, the EXACT restatement of the header's statements,
the fp64 water with the profile in it, the profiles and the population the bound is derived on, and PROFILE_BOUND.  It composes the
existing modules: the finite-depth water is tests/sea_depth_reference.py's, the closed loop tests/closed_loop_reference.py's.

Importing this module registers `"shear"` in resident_harness.ENTRIES and RAW_EXTRAS: the signature is the _fd entry's
(tests/sea_ensemble_harness.py's `launch` and `raw_ens` take entry="shear").

THE RESTATEMENT (`profile_exact`): include/hydro.h's statements one by one - the subtraction, the product, the two clamps, the FMA of
each component - each statement's REAL result rounded once to fp32.  The real results are formed in fp64 where fp64 holds them
exactly (the product of two fp32 values always; the difference and the FMA whenever the exponents are close), and a result that
lands on a midpoint of two fp32 neighbours after the fp64 rounding - the only place where rounding twice could differ from rounding
once - is formed over again with fractions.Fraction and rounded from there.  `drop_last=True` leaves the last knot away: the
restatement a kernel whose loop ends one trip early would meet.

THE BOUND.  `profile_errors` gives the largest distance of a restated (or device) profile to `CurrentProfile.velocity`, the fp64
piecewise-linear profile at the same fp32 zc, in units of 2^-24 of max_l |V_l| (the largest component of any knot).  Over
`population()` - bodies ON every knot, one fp32 neighbour either side of every knot, between the knots, below the bed, above the
surface - for `turning_profile(K)`, K = 1, 2, 3, 16 (a power law over H = 9 m whose heading turns through 120 degrees from the bed
to the surface, with a small vertical part), the restatement gives E = 2.75 (K = 1: 0, 2: 2.75, 3: 1.37, 16: 0.54 - the fewer the
knots, the larger |D_l| against max |V|, and the rounding of t_l and of inv_l is carried by |D_l|; printed by
tests/test_current_profile.py), so PROFILE_BOUND = the next power of two at or above 2 E = 5.5, which is 8.  The factor 2 is
DESIGN.md section 17's allowance.  The device is not held to it: it is held to the restatement's bits.
"""
import contextlib
from fractions import Fraction

import numpy as np

import resident_harness as rh
import sea_depth_reference as sdr  # noqa: F401  (registers "fd")
import sea_reference as sr
from silver2_isaacsim_amd.sea import CurrentProfile

rh.ENTRIES["shear"] = ("step_fused_tiled_multi_shear", rh.ENTRIES["stat"][1])
rh.RAW_EXTRAS["shear"] = rh.RAW_EXTRAS["stat"]

F32 = np.float32
PROFILE_BOUND = 8.0               # units of 2^-24 of max |V| (derived above, on the host)
DEPTH = sdr.DEPTH                 # m: the depth the designed sea of tests/sea_depth_reference.py lives in
KNOTS = (1, 2, 3, 16)


def turning_profile(knots=16, depth=DEPTH, speed=1.2):
    """`knots` knots of a 1/7 power law over `depth` whose heading turns from 200 degrees at the bed to 320 at the surface, with a
    vertical part of a tenth - every D_l has three non-zero components.  One knot: the surface value at z = -depth / 2."""
    if knots == 1:
        return CurrentProfile([-0.5 * depth], [[0.9, -0.4, 0.1]])
    frac = (np.arange(knots) / (knots - 1.0)) ** 4
    mag = speed * (0.05 + frac) ** (1.0 / 7.0)
    hd = np.radians(200.0 + 120.0 * np.arange(knots) / (knots - 1.0))
    return CurrentProfile(-depth * (1.0 - frac), np.stack([mag * np.cos(hd), mag * np.sin(hd), 0.1 * mag * np.cos(3.0 * hd)], axis=1))


def without_last_knot(profile):
    return CurrentProfile(profile.z[:-1], profile.v[:-1])


def population(profile, depth=DEPTH, extra=40):
    """(n, 13) fp32 states within 40 m of the origin: a body ON every knot, one fp32 neighbour below and above every knot, one
    between every two knots, then `extra` spread over: below the bed, on the bed, mid-depth, at the surface, above it."""
    zk = profile.z.astype(F32)
    z = [zk, np.nextafter(zk, F32(-np.inf)), np.nextafter(zk, F32(np.inf)), (0.5 * (profile.z[1:] + profile.z[:-1])).astype(F32)]
    rng = np.random.default_rng(34)
    kind = np.arange(extra) % 5
    z.append(np.where(kind == 0, rng.uniform(-1.5 * depth, -1.02 * depth, extra),
                      np.where(kind == 1, -depth, np.where(kind == 2, rng.uniform(-0.99 * depth, -0.01 * depth, extra),
                                                           np.where(kind == 3, rng.uniform(-0.3, 0.3, extra), rng.uniform(0.5, 2.0, extra))))).astype(F32))
    z = np.concatenate(z)
    st = np.zeros((len(z), 13), F32)
    st[:, 0:2] = rng.uniform(-40.0, 40.0, (len(z), 2))
    st[:, 2] = z
    st[:, 6] = 1.0
    st[:, 7:10] = rng.uniform(-0.5, 0.5, (len(z), 3))
    return st


def clamped_depth(pz, eta, depth):
    """zc = max(min(p_z - eta, 0), -h) in fp32, h rounded once (min and max return the number)."""
    with np.errstate(invalid="ignore"):
        z_rel = np.asarray(pz, F32) - np.asarray(eta, F32)
        zc = np.where(np.isnan(z_rel), F32(0.0), np.minimum(z_rel, F32(0.0))).astype(F32)
    return np.maximum(zc, F32(-depth))


def _fl32(x: Fraction):
    """The fp32 value nearest the real number x, ties to even (x within fp32's normal range or 0)."""
    c = F32(float(x))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        d = abs(Fraction(float(cand)) - x)
        even = (int(np.asarray(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, cand, even)
    return best[1]


def _once(r64, exact):
    """fp64 results `r64` of one statement as fp32, rounded ONCE from the real result: elements that sit on a midpoint of two fp32
    neighbours are formed over again by `exact(index) -> Fraction`."""
    r64 = np.asarray(r64, np.float64)
    r32 = r64.astype(F32)
    for side in (np.inf, -np.inf):
        mid = 0.5 * (r32.astype(np.float64) + np.nextafter(r32, F32(side)).astype(np.float64))
        for i in np.flatnonzero((r64 == mid) & (r32.astype(np.float64) != r64)):
            r32[i] = _fl32(exact(int(i)))
    return r32


def profile_exact(profile, zc, drop_last=False):
    """P (n, 3) fp32 at the fp32 depths `zc`: include/hydro.h's "Current profile", every statement's real result rounded once."""
    if drop_last:
        profile = without_last_knot(profile)
    v0, z, inv, d = profile.table()
    zc = np.asarray(zc, F32).reshape(-1)
    fr = lambda a: Fraction(float(a))  # noqa: E731
    p = [np.full(zc.shape, v0[i], F32) for i in range(3)]
    for l in range(len(z)):  # noqa: E741
        diff = _once(zc.astype(np.float64) - float(z[l]), lambda i: fr(zc[i]) - fr(z[l]))
        prod = _once(diff.astype(np.float64) * float(inv[l]), lambda i: fr(diff[i]) * fr(inv[l]))
        with np.errstate(invalid="ignore"):
            t = np.minimum(np.maximum(prod, F32(0.0)), F32(1.0))
        for i in range(3):
            pi = p[i]
            p[i] = _once(float(d[l, i]) * t.astype(np.float64) + pi.astype(np.float64), lambda j: fr(d[l, i]) * fr(t[j]) + fr(pi[j]))
    return np.stack(p, axis=-1)


def profile_errors(profile, zc, p32):
    """The largest distance of the fp32 profile `p32` at the fp32 depths `zc` to the fp64 piecewise-linear profile, in units of 2^-24
    of max |V|."""
    scale = np.abs(profile.v).max()
    return float((np.abs(np.asarray(p32, np.float64) - profile.velocity(np.asarray(zc, np.float64))) / (sr.ULP * scale)).max())


def water(sea, profile, px, py, pz, step, dt):
    """(eta (n,), u (n, 3)) in fp64: tests/sea_depth_reference.py's water of the finite-depth `sea`, the profile added at
    zc = clip(p_z - eta, -h, 0)."""
    eta, u = sdr.water(sea, px, py, pz, step, dt)
    with np.errstate(invalid="ignore"):
        zc = np.maximum(np.minimum(np.nan_to_num(np.asarray(pz, np.float64) - eta, nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0), -sea.depth)
    return eta, u + profile.velocity(zc)


@contextlib.contextmanager
def sheared_water(profile):
    """While it is open, the fp64 closed loop of tests/closed_loop_reference.py reads its water from `water` above for every sea that
    has a depth; any other sea as before."""
    before = sr.water
    sr.water = lambda sea, px, py, pz, step, dt: water(sea, profile, px, py, pz, step, dt) if getattr(sea, "depth", None) is not None \
        else before(sea, px, py, pz, step, dt)
    try:
        yield
    finally:
        sr.water = before


def drifting_cubes(depth=20.0, levels=(-2.0, -8.0, -14.0, -19.0)):
    """tests/designed_populations.py's drift scene four times over: neutrally buoyant 0.5 m cubes at rest at `levels`, 10 m apart."""
    from designed_populations import drift_scene
    st, pv, pr, _ = drift_scene()
    st, pv, pr = (np.repeat(a, len(levels), axis=0) for a in (st, pv, pr))
    st[:, 0] = 10.0 * np.arange(len(levels))
    st[:, 2] = levels
    return st, pv, pr
