"""The mooring line of hydro_step_fused_tiled_multi_moor (include/hydro.h, "Mooring") restated in fp64 NumPy: the reference of
tests/test_mooring.py and tests/test_mooring_gpu.py.  No device, no library, nothing of silver2_isaacsim_amd.mooring.

A record is an (n, 9) array [a(3) | b(3) | L0 | k | c]: anchor (world), fairlead (body frame), unstretched length, stiffness,
damping.  For a body [p | q | v | omega]:

    r  = R b                e = (a - p) - r             l = |e|             x = l - L0          taut: x > 0
    u  = v + omega x r      un = u . e / l              T = max(0, k x - c un)
    F  = T e / l            W = (F, r x F)              only where the body has a line (k > 0 or c > 0), it is taut and T > 0

The line sees the TRUE state; in a step W is added behind the applied wrench, the pose hold and the bed, in front of the
integrator.

THE DECISION x > 0 is where the model is discontinuous when c > 0 (a line that comes taut while the fairlead runs away from
the anchor meets the damper at full strength), and x = l - L0 cancels, so a reference that decides in fp64 and a kernel that
decides in fp32 may differ by a whole damper force on a line within a rounding of its length.  With c = 0 the tension is
continuous there.  `taut(..., rec)` decides in fp64; `taut_fp32` restates the kernel's decision in NumPy float32 (with a
correctly rounded seed of the reciprocal square root), and `wrench(..., taut=)` takes either.
"""
import numpy as np

from rigid_reference import cross_fp32, cross_scale, fma32, point_velocity_fp32, point_velocity_scale, rot, rot_fp32, rot_magnitudes, rsqrt_nr32

ULP = 2.0 ** -24
PROBE_BOUND = 2.0             # units of 2^-24 of wrench_scales: tests/test_mooring_gpu.py's bound (its docstring)
FIELDS = 9


def has_line(rec):
    rec = np.asarray(rec)
    return (rec[:, 7] > 0) | (rec[:, 8] > 0)


def geometry(rec, state):
    """(r, e, l, x, u, un) in fp64: arm, fairlead -> anchor, its length, the stretch, the fairlead's velocity, its approach speed."""
    m, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    r = np.einsum("nab,nb->na", rot(st[:, 3:7]), m[:, 3:6])
    e = (m[:, 0:3] - st[:, 0:3]) - r
    l = np.sqrt((e * e).sum(axis=1))
    u = st[:, 7:10] + np.cross(st[:, 10:13], r)
    with np.errstate(divide="ignore", invalid="ignore"):
        un = (u * e).sum(axis=1) / l
    return r, e, l, l - m[:, 6], u, un


def taut(rec, state):
    """(n,) bool: the body has a line and it is stretched, x > 0, decided in fp64."""
    return has_line(rec) & (geometry(rec, state)[3] > 0)


def tension(rec, state, taut=None):
    """(n,) T in fp64, 0 where the line adds nothing; `taut`: which lines are stretched, default decided in fp64."""
    m = np.asarray(rec, np.float64)
    _, _, _, x, _, un = geometry(rec, state)
    on = (has_line(rec) & (x > 0)) if taut is None else np.asarray(taut, bool)
    with np.errstate(invalid="ignore"):
        T = np.maximum(0.0, m[:, 7] * x - m[:, 8] * un)
    return np.where(on & (T > 0), T, 0.0)


def wrench(rec, state, taut=None):
    """(n, 6) W in fp64."""
    r, e, l, _, _, _ = geometry(rec, state)
    T = tension(rec, state, taut)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        F = np.where((T > 0)[:, None], (T / l)[:, None] * e, 0.0)
        M = np.where((T > 0)[:, None], np.cross(r, F), 0.0)           # a lane that adds nothing: +0, whatever its arm (NaN x 0 is NaN)
    return np.concatenate([F, M], axis=1)


def wrench_scales(rec, state, taut=None, contributing=None):
    """What an fp32 evaluation of W rounds against, per body and component (n, 6): the sum of the magnitudes of the terms that
    form it; 0 for a body whose line adds nothing (`contributing` (n,) bool overrides that decision: the scale of a line at
    the tie, whichever way it falls).  With R^ the matrix of term magnitudes of R (rigid_reference.rot_magnitudes) and
        r^_i = sum_j R^_ij |b_j|            e^_i = |a_i| + |p_i| + r^_i             l^ = |e^|  (>= l; what l rounds against)
        u^_x = |v_x| + |omega_y| r^_z + |omega_z| r^_y  (cyclic)                   u^ = sum_i u^_i e^_i / l
        T^   = k (l^ + L0) + c u^           - NOT T: x = l - L0 cancels, and the rounding of l reaches T whatever is left of x
        F^_i = T^ e^_i / l                  M^ = r^ x^ F^ with every product of the cross product counted positive"""
    m, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    _, _, l, _, _, _ = geometry(rec, state)
    on = tension(rec, state, taut) > 0 if contributing is None else np.asarray(contributing, bool)
    rh = np.einsum("nab,nb->na", rot_magnitudes(st[:, 3:7]), np.abs(m[:, 3:6]))
    eh = np.abs(m[:, 0:3]) + np.abs(st[:, 0:3]) + rh
    lh = np.sqrt((eh * eh).sum(axis=1))
    uh = point_velocity_scale(st[:, 7:10], st[:, 10:13], rh)
    safe_l = np.where(on, l, 1.0)
    unh = (uh * eh).sum(axis=1) / safe_l
    Th = m[:, 7] * (lh + m[:, 6]) + m[:, 8] * unh
    Fh = Th[:, None] * eh / safe_l[:, None]
    return np.concatenate([Fh, cross_scale(rh, Fh)], axis=1) * on[:, None]


def _fp32_terms(rec, state):
    """The header's operations in NumPy float32, in its order: (r, e, inv, x, T) - lists of (n,) float32 arrays."""
    f32 = np.float32
    m, st = np.asarray(rec, f32), np.asarray(state, f32)
    R = rot_fp32(st[:, 3:7])
    b = [m[:, 3], m[:, 4], m[:, 5]]
    r = [fma32(R[i][2], b[2], fma32(R[i][1], b[1], R[i][0] * b[0])) for i in range(3)]
    e = [(m[:, i] - st[:, i]) - r[i] for i in range(3)]
    l2 = fma32(e[2], e[2], fma32(e[1], e[1], e[0] * e[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = rsqrt_nr32(l2)
        l = l2 * inv
        x = l - m[:, 6]
        ux, uy, uz = point_velocity_fp32(st, r)
        un = fma32(uz, e[2], fma32(uy, e[1], ux * e[0])) * inv
        T = fma32(m[:, 7], x, -(m[:, 8] * un))
        T = np.where(T > 0, T, f32(0))                             # max(0, .) that gives 0 for a NaN, as the hardware's does
    return r, e, inv, x, T


def taut_fp32(rec, state):
    """(n,) bool: the kernel's own decision - a line, and x > 0 in the fp32 operations include/hydro.h lists."""
    return has_line(np.asarray(rec, np.float32)) & (_fp32_terms(rec, state)[3] > 0)


def wrench_fp32_emulated(rec, state):
    """(n, 6) W by the operations of include/hydro.h in NumPy float32, in the header's order: what the kernel computes but for
    the seed of the reciprocal square root and the rare double rounding of fma32."""
    f32 = np.float32
    r, e, inv, x, T = _fp32_terms(rec, state)
    on = has_line(np.asarray(rec, f32)) & (x > 0) & (T > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ti = T * inv
        F = [ti * e[i] for i in range(3)]
        M = cross_fp32(r, F)
    return np.where(on[:, None], np.stack(F + M, axis=1), f32(0)).astype(f32)
