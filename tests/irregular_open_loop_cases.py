"""What tests/test_sea_irregular_open_loop.py (no device) and tests/test_sea_irregular_open_loop_gpu.py share: the population, the
seas and the fp64 wrench that says whether an identity between two launches means something.

THE POPULATION (`near_surface`): the first 321 bodies of the designed population (designed_populations.hold_pop: every attitude,
slabs up to 1:10, |v| up to 5 m/s, 5 % of the bodies out to 1e4 m in x and y), with every body whose centre is above
z = -0.05 m or deeper than 2 m moved, in z only, to a depth between -2 m and -0.25 m: submerged and surface-piercing buoys within |p_z| < 2 m, where the waves
of a Tp = 7 s sea and a depth of 9 m are both felt.  (The wrench takes the water's velocity only while the body's centre is under
the local surface: a body with its centre above it feels the depth through nothing.  The bodies that pierce the surface here do so from below.)
THE SEAS: tests/sea_ensemble_harness.py's members (JONSWAP, Hs 0.8 .. 1.8 m, Tp 7 s, cos^2 spreading, each on a current of its own).
The lone spectrum is member 0; the finite-depth sea is the same components taken as given at h = 9 m (tests/sea_depth_reference.py).
THE FP64 WRENCH (`fp64_wrench`): hydro_oracle.step_wrench on the state relative to the fp64 water of sea_depth_reference.water at
`time` seconds; `moved` counts the bodies on which two such wrenches differ by more than 10 times the project's gate of 1e-5, in
hydro_oracle.wrench_error's measure - no device, no library.
"""
import numpy as np

import sea_depth_reference as sdr
import sea_ensemble_harness as seh
from oracle import hydro_oracle as ho
from resident_harness import DT, G, RHO
from sea_reference import relative

N = 321
SIZES = (1, 63, 64, 65, 257)                                      # the last tile has one live lane; 257 is a second block
ENSEMBLE_CASES = ((200, 1), (200, 2), (321, 1), (321, 2))         # (n, tiles_per_sea): at 1 the four waves of a block read four members
COUNTS = (9, 10, 11, 63, 64)                                      # every remainder of the unroll by four, and the full table
DEPTH = sdr.DEPTH                                                 # 9 m: kappa_p h = 0.98 at Tp = 7 s
FAR = 1e6                                                         # m: deep water for every component of the members
TIMES = (0.0, DT, 7.0 * DT, 1e6 * DT, 0.123456789)                # fp64 products step * DT, and one that is no multiple of DT
GATE = 1e-5                                                       # the project's gate on hydro_oracle.wrench_error
MOVED = 10.0 * GATE                                               # a launch through the wrong water misses the gate tenfold


def near_surface(st, pv, params):
    """(state, prev, {coeff: params}) of the first N bodies, moved in z as the module's docstring says."""
    st, pv = st[:N].copy(), pv[:N].copy()
    rng = np.random.default_rng(33)
    z = st[:, 2].astype(np.float64)
    away = (z > -0.05) | (z < -2.0)
    st[:, 2] = np.where(away, rng.uniform(-2.0, -0.25, N), z).astype(np.float32)
    return st, pv, {k: v[:N].copy() for k, v in params.items()}


def lone(count=64, member=0):
    return seh.members(count)[member]


def at_depth(sea, depth=DEPTH):
    """A spectrum, or every member of an ensemble, with its components taken as given at `depth`."""
    if hasattr(sea, "members"):
        return type(sea)([sdr.with_depth(m, depth) for m in sea.members], sea.bodies_per_sea)
    return sdr.with_depth(sea, depth)


def member_of(sea, body):
    return sea.members[body // sea.bodies_per_sea] if hasattr(sea, "members") else sea


def fp64_wrench(sea, st, pv, pr, time, semantics="numba"):
    """(n, 6) fp64: the wrench of the first len(st) bodies in `sea` (None: still water; a spectrum or an ensemble, with or without
    a depth) at `time` seconds."""
    n = len(st)
    eta, u = np.zeros(n), np.zeros((n, 3))
    if sea is not None:
        blocks = [(0, n, sea)] if not hasattr(sea, "members") else \
            [(a, min(a + sea.bodies_per_sea, n), sea.members[a // sea.bodies_per_sea]) for a in range(0, n, sea.bodies_per_sea)]
        for a, b, member in blocks:
            eta[a:b], u[a:b] = sdr.water(member, st[a:b, 0], st[a:b, 1], st[a:b, 2], 1, time)
    s_rel, pv_rel = relative(st, pv, eta, u)
    f, t, _ = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT, semantics=semantics)
    return np.concatenate([f, t], axis=1)


def moved(a, b, pr):
    """(the fraction of bodies on which the fp64 wrenches a and b differ by more than MOVED, whether some body of EVERY tile does)."""
    n = len(a)
    d = ho.wrench_error(a[:, 0:3], a[:, 3:6], b[:, 0:3], b[:, 3:6], pr[:n], RHO, G) > MOVED
    return float(d.mean()), all(d[t:t + 64].any() for t in range(0, n, 64))
