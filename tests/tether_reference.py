"""The tether of hydro_step_fused_tiled_multi_teth (include/hydro.h, "Tether") restated in fp64 NumPy: the reference of
tests/test_tether.py and tests/test_tether_gpu.py.  No device, no library, nothing of silver2_isaacsim_amd.tether.

A record is an (n, 7) array [b(3) | L0 | k | c | partner]: this body's fairlead (body frame), unstretched length, stiffness,
damping, and the partner as a lane of the body's own tile of 64 (body 64 (i // 64) + (int(partner) & 63)).  For a body
[p | q | v | omega] and its partner (primed):

    r  = R b        P = p + r       U = v + omega x r
    e  = P' - P     l = |e|         x = l - L0          taut: x > 0
    dU = U' - U     rate = dU . e / l                   T = max(0, k x + c rate)
    F  = T e / l    W = (F, r x F)  only where the body has a tether (k > 0 or c > 0), it is taut and T > 0

A partner >= n (a lane of the last tile that holds no body) answers P' = U' = 0, as a masked lane of the wavefront does.
The tether sees the TRUE state; in a step W is added behind the mooring line's wrench, in front of the integrator.

THE DECISION x > 0 is where the model is discontinuous when c > 0, and x = l - L0 cancels: `taut(rec, state)` decides in fp64;
`taut_fp32` restates the kernel's decision in NumPy float32 (with a correctly rounded seed of the reciprocal square root),
and `wrench(..., taut=)` takes either.
"""
import numpy as np

from rigid_reference import cross_fp32, cross_scale, fma32, point_velocity_fp32, point_velocity_scale, rot, rot_fp32, rot_magnitudes, rsqrt_nr32

ULP = 2.0 ** -24
PROBE_BOUND = 2.0             # units of 2^-24 of wrench_scales (tests/test_tether.py's docstring)
FIELDS = 7
TILE = 64


def has_tether(rec):
    rec = np.asarray(rec)
    return (rec[:, 4] > 0) | (rec[:, 5] > 0)


def partner(rec):
    """(n,) the body each record names."""
    rec = np.asarray(rec)
    i = np.arange(len(rec))
    return (i // TILE) * TILE + (rec[:, 6].astype(np.int64) & (TILE - 1))


def _from_partner(rec, a):
    """a[partner], zeros where the partner is no body."""
    j = partner(rec)
    ok = j < len(a)
    out = np.zeros_like(a)
    out[ok] = a[j[ok]]
    return out


def geometry(rec, state):
    """(r, e, l, x, dU, rate) in fp64: arm, fairlead -> partner's fairlead, its length, the stretch, the partner's fairlead
    velocity against this one's, the rate at which the two part."""
    t, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    r = np.einsum("nab,nb->na", rot(st[:, 3:7]), t[:, 0:3])
    P = st[:, 0:3] + r
    U = st[:, 7:10] + np.cross(st[:, 10:13], r)
    e = _from_partner(rec, P) - P
    dU = _from_partner(rec, U) - U
    l = np.sqrt((e * e).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = (dU * e).sum(axis=1) / l
    return r, e, l, l - t[:, 3], dU, rate


def taut(rec, state):
    """(n,) bool: the body has a tether and it is stretched, x > 0, decided in fp64."""
    return has_tether(rec) & (geometry(rec, state)[3] > 0)


def tension(rec, state, taut=None):
    """(n,) T in fp64, 0 where the tether adds nothing; `taut`: which are stretched, default decided in fp64."""
    t = np.asarray(rec, np.float64)
    _, _, _, x, _, rate = geometry(rec, state)
    on = (has_tether(rec) & (x > 0)) if taut is None else np.asarray(taut, bool)
    with np.errstate(invalid="ignore"):
        T = np.maximum(0.0, t[:, 4] * x + t[:, 5] * rate)
    return np.where(on & (T > 0), T, 0.0)


def wrench(rec, state, taut=None):
    """(n, 6) W in fp64."""
    r, e, l, _, _, _ = geometry(rec, state)
    T = tension(rec, state, taut)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        F = np.where((T > 0)[:, None], (T / l)[:, None] * e, 0.0)
        M = np.where((T > 0)[:, None], np.cross(r, F), 0.0)           # a lane that adds nothing: +0, whatever its arm (NaN x 0 is NaN)
    return np.concatenate([F, M], axis=1)


def _magnitudes(rec, state):
    """(r^, P^, U^) per body: the sums of the magnitudes of the terms that form the arm, the fairlead and its velocity."""
    t, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    rh = np.einsum("nab,nb->na", rot_magnitudes(st[:, 3:7]), np.abs(t[:, 0:3]))
    return rh, np.abs(st[:, 0:3]) + rh, point_velocity_scale(st[:, 7:10], st[:, 10:13], rh)


def wrench_scales(rec, state, taut=None, contributing=None):
    """What an fp32 evaluation of W rounds against, per body and component (n, 6): the sum of the magnitudes of the terms that
    form it; 0 for a body whose tether adds nothing (`contributing` (n,) bool overrides that decision: the scale of a line at
    the tie, whichever way it falls).  With r^, P^ = |p| + r^ and U^ the term magnitudes of arm, fairlead and fairlead velocity
    (as in mooring_reference.wrench_scales), of this body and, primed, of its partner:
        e^_i  = P'^_i + P^_i          l^ = |e^|  (>= l; what l rounds against)
        dU^_i = U'^_i + U^_i          |dU^| = sum_i dU^_i e^_i / l      what the rate rounds against
        T^    = k (l^ + L0) + c |dU^|  - NOT T: x = l - L0 cancels, and the rounding of l reaches T whatever is left of x
        F^_i  = T^ e^_i / l           M^ = r^ x^ F^ with every product of the cross product counted positive"""
    t = np.asarray(rec, np.float64)
    _, _, l, _, _, _ = geometry(rec, state)
    on = tension(rec, state, taut) > 0 if contributing is None else np.asarray(contributing, bool)
    rh, Ph, Uh = _magnitudes(rec, state)
    eh = _from_partner(rec, Ph) + Ph
    dUh = _from_partner(rec, Uh) + Uh
    lh = np.sqrt((eh * eh).sum(axis=1))
    safe_l = np.where(on & (l > 0), l, 1.0)
    rate_h = (dUh * eh).sum(axis=1) / safe_l
    Th = t[:, 4] * (lh + t[:, 3]) + t[:, 5] * rate_h
    Fh = Th[:, None] * eh / safe_l[:, None]
    return np.concatenate([Fh, cross_scale(rh, Fh)], axis=1) * on[:, None]


def tension_scale(rec, state, taut=None, contributing=None):
    """(n,) T^ of wrench_scales: what the tension rounds against; 0 where the tether adds nothing."""
    t = np.asarray(rec, np.float64)
    _, _, l, _, _, _ = geometry(rec, state)
    on = tension(rec, state, taut) > 0 if contributing is None else np.asarray(contributing, bool)
    _, Ph, Uh = _magnitudes(rec, state)
    eh, dUh = _from_partner(rec, Ph) + Ph, _from_partner(rec, Uh) + Uh
    safe_l = np.where(on & (l > 0), l, 1.0)
    return (t[:, 4] * (np.sqrt((eh * eh).sum(axis=1)) + t[:, 3]) + t[:, 5] * (dUh * eh).sum(axis=1) / safe_l) * on


def _fp32_terms(rec, state):
    """The header's operations in NumPy float32, in its order: (r, e, inv, x, T) - lists of (n,) float32 arrays."""
    f32 = np.float32
    t, st = np.asarray(rec, f32), np.asarray(state, f32)
    R = rot_fp32(st[:, 3:7])
    b = [t[:, 0], t[:, 1], t[:, 2]]
    r = [fma32(R[i][2], b[2], fma32(R[i][1], b[1], R[i][0] * b[0])) for i in range(3)]
    P = [st[:, i] + r[i] for i in range(3)]
    U = point_velocity_fp32(st, r)
    e = [_from_partner(rec, P[i]) - P[i] for i in range(3)]
    dU = [_from_partner(rec, U[i]) - U[i] for i in range(3)]
    l2 = fma32(e[2], e[2], fma32(e[1], e[1], e[0] * e[0]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = rsqrt_nr32(l2)
        l = l2 * inv
        x = l - t[:, 3]
        rate = fma32(dU[2], e[2], fma32(dU[1], e[1], dU[0] * e[0])) * inv
        T = fma32(t[:, 4], x, t[:, 5] * rate)
        T = np.where(T > 0, T, f32(0))                             # max(0, .) that gives 0 for a NaN, as the hardware's does
    return r, e, inv, x, T


def taut_fp32(rec, state):
    """(n,) bool: the kernel's own decision - a tether, and x > 0 in the fp32 operations include/hydro.h lists."""
    return has_tether(np.asarray(rec, np.float32)) & (_fp32_terms(rec, state)[3] > 0)


def wrench_fp32_emulated(rec, state, with_tension=False):
    """(n, 6) W by the operations of include/hydro.h in NumPy float32, in the header's order: what the kernel computes but for
    the seed of the reciprocal square root and the rare double rounding of fma32.  with_tension: (W, T), T (n,) float32."""
    f32 = np.float32
    r, e, inv, x, T = _fp32_terms(rec, state)
    on = has_tether(np.asarray(rec, f32)) & (x > 0) & (T > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ti = T * inv
        F = [ti * e[i] for i in range(3)]
        M = cross_fp32(r, F)
    W = np.where(on[:, None], np.stack(F + M, axis=1), f32(0)).astype(f32)
    return (W, np.where(on, T, f32(0)).astype(f32)) if with_tension else W
