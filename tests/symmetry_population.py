"""The population of the symmetry tests' later rungs (tether, net, link tensions, spread, irregular sea), built without a device:
shared by tests/test_symmetry.py, which asserts what it is made of, and tests/test_symmetry_gpu.py, which runs it.

It is the population of tests/test_mooring_spread_gpu.py - the first 321 bodies of tether_net_population.net_population with
mooring_population.line_population and mooring_spread_population.spread_population over them - RESEATED: designed_populations.
tilted_boxes moves four bodies in five, in z only, onto ONE corner, because the bed's corner sum is the one order-sensitive sum on
the device (tests/test_symmetry_gpu.py) and 59 % of the population as drawn stands on two or more corners.  The mooring lines and
the spread are drawn anew from the moved states (every anchored line is built from its own body's state; the ties at bodies
0 .. 7 are not moved and keep their records); the controller's targets follow the bodies in z.  The tether net is NOT drawn anew:
its lines join two bodies, and the moved population keeps enough of them pulling (asserted in tests/test_symmetry.py).

For the rungs that know a depth (finite-depth sea, sheared current) the module also says in which water the population stands
(`FD_DEPTH`, `fd_sea`, `fd_ensemble`), measures its water column by the fp64 reference (`column_shares`) and builds the probe
population that holds a body in every knot interval of a profile (`knot_population`).
"""
import numpy as np

from designed_populations import tilted_boxes
from mooring_population import line_population
from mooring_spread_population import spread_population
from tether_net_population import net_for, net_population

N = 321
NET_LAYERS = 2                                                    # the layers of the net the resident tests run
SPREAD_LAYERS = 3                                                 # "the spread of three": layer 3 of the designed spread is zeros


def reseated_population():
    """dict(st, drawn (the states before reseating), pv, params {f32, f16}, net (322, 28), spread (321, 36), lines (321, 9), groups):
    see the module's docstring.  The applied wrench and the control record are the fixtures' (designed_populations.bed_pop); the
    caller moves the targets with `follow`."""
    st, pv, pr, net, groups = net_population()
    st, pv, pr = st[:N], pv[:N], pr[:N]
    moved, _, _ = tilted_boxes(st, pv, pr)
    rec = line_population(st, pr)
    changed = moved[:, 2] != st[:, 2]
    lines = np.where(changed[:, None], line_population(moved, pr), rec)
    spread = spread_population(moved, pr, lines)
    p16 = pr.copy()
    p16[:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    return dict(st=moved, drawn=st, pv=pv, params={"f32": pr, "f16": p16}, net=net, spread=spread, lines=lines, groups=groups)


def follow(ctl, drawn, moved):
    """The control record with its targets moved in z as the bodies were, so that the law's terms keep their sizes."""
    out = ctl.copy()
    out[:, 2] = (ctl[:, 2].astype(np.float64) + (moved[:, 2].astype(np.float64) - drawn[:, 2])).astype(np.float32)
    return out


def net_of(pop, n, layers=NET_LAYERS):
    """The net of the first n bodies: tether_net_population.net_for."""
    return net_for(pop["net"], n, layers)


# ---- the water column of the finite-depth and sheared-current rungs ---------------------------------------------------------------------
# The reseated population lies between z = -3.6 m and z = -2.0 m, over the bed of the bed tests at z = -3 m: in water of THAT depth
# 70 % of it sits strictly inside the column and 28 .. 30 % on the clamp zc = -h (tests/test_symmetry.py asserts both and prints
# the rest).  Nobody reaches the surface clamp zc = 0 at any depth - the bodies are two metres down and the designed sea's
# amplitudes sum to less - so the probes also run on sea_depth_reference.population(), which covers the column by construction,
# and on `knot_population`, which puts a body into every knot interval.
FD_DEPTH = 3.0


def fd_sea(components=64, depth=FD_DEPTH):
    """sea_depth_reference.designed_sea in the depth the resident rungs run at."""
    import sea_depth_reference as sdr
    return sdr.designed_sea(components, depth)


def fd_ensemble(waves, n, tiles_per_sea, depth=FD_DEPTH):
    """sea_ensemble_harness.ensemble(waves, n, tiles_per_sea), every member given `depth`."""
    import sea_depth_reference as sdr
    import sea_ensemble_harness as seh
    from silver2_isaacsim_amd.sea import SeaEnsemble
    ens = seh.ensemble(waves, n, tiles_per_sea)
    return SeaEnsemble([sdr.with_depth(m, depth) for m in ens.members], ens.bodies_per_sea)


def column_shares(sea, profile, st, step, dt):
    """By the fp64 reference: dict(inside, surface, bed: the shares of bodies with -h < zc < 0, zc = 0, zc = -h; intervals: the
    number of the profile's knot intervals that hold a body strictly inside; eta: whether eta is non-zero for every body)."""
    import sea_depth_reference as sdr
    h = sea.depth
    eta, _ = sdr.water(sea, st[:, 0], st[:, 1], st[:, 2], step, dt)
    zc = np.clip(st[:, 2].astype(np.float64) - eta, -h, 0.0)
    inside = (zc > -h) & (zc < 0.0)
    held = np.histogram(zc[inside], bins=profile.z)[0] if profile is not None and profile.knots > 1 else np.zeros(0, int)
    return dict(inside=float(inside.mean()), surface=float((zc == 0.0).mean()), bed=float((zc == -h).mean()), intervals=int((held > 0).sum()),
                eta=bool((eta != 0.0).all()))


def knot_population(profile, sea, step, dt, per_interval=2):
    """(n, 13) fp32 states within 40 m of the origin with `per_interval` bodies in EVERY knot interval of `profile` at `step`: eta
    does not depend on p_z, so p_z = eta(x, y) + (a point of the interval) in fp64, rounded once.  The lowest interval of the
    16-knot turning profile is 0.06 mm wide at h = 3 m; an fp32 p_z near 3 m resolves 0.2 micrometres."""
    import sea_depth_reference as sdr
    rng = np.random.default_rng(35)
    lo, hi = profile.z[:-1], profile.z[1:]
    frac = (np.arange(per_interval) + 1.0) / (per_interval + 1.0)
    zc = (lo[:, None] + frac[None, :] * (hi - lo)[:, None]).reshape(-1)
    st = np.zeros((len(zc), 13), np.float32)
    st[:, 0:2] = rng.uniform(-40.0, 40.0, (len(zc), 2))
    eta, _ = sdr.water(sea, st[:, 0], st[:, 1], np.zeros(len(zc)), step, dt)
    st[:, 2] = (eta + zc).astype(np.float32)
    st[:, 6] = 1.0
    st[:, 7:10] = rng.uniform(-0.5, 0.5, (len(zc), 3))
    return st
