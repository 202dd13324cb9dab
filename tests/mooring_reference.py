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

from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io

import sea_reference as sr
import seabed_reference as br

ULP = 2.0 ** -24
FIELDS = 9


def has_line(rec):
    rec = np.asarray(rec)
    return (rec[:, 7] > 0) | (rec[:, 8] > 0)


def geometry(rec, state):
    """(r, e, l, x, u, un) in fp64: arm, fairlead -> anchor, its length, the stretch, the fairlead's velocity, its approach speed."""
    m, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    r = np.einsum("nab,nb->na", br._rot(st[:, 3:7]), m[:, 3:6])
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
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where((T > 0)[:, None], (T / l)[:, None] * e, 0.0)
    return np.concatenate([F, np.cross(r, F)], axis=1)


def wrench_scales(rec, state, taut=None, contributing=None):
    """What an fp32 evaluation of W rounds against, per body and component (n, 6): the sum of the magnitudes of the terms that
    form it; 0 for a body whose line adds nothing (`contributing` (n,) bool overrides that decision: the scale of a line at
    the tie, whichever way it falls).  With R^ the matrix of term magnitudes of R (seabed_reference) and
        r^_i = sum_j R^_ij |b_j|            e^_i = |a_i| + |p_i| + r^_i             l^ = |e^|  (>= l; what l rounds against)
        u^_x = |v_x| + |omega_y| r^_z + |omega_z| r^_y  (cyclic)                   u^ = sum_i u^_i e^_i / l
        T^   = k (l^ + L0) + c u^           - NOT T: x = l - L0 cancels, and the rounding of l reaches T whatever is left of x
        F^_i = T^ e^_i / l                  M^ = r^ x^ F^ with every product of the cross product counted positive"""
    m, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    _, _, l, _, _, _ = geometry(rec, state)
    on = tension(rec, state, taut) > 0 if contributing is None else np.asarray(contributing, bool)
    x, y, z, w = (np.abs(st[:, 3 + i]) for i in range(4))
    Rh = np.empty((len(st), 3, 3))
    Rh[:, 0, 0], Rh[:, 1, 1], Rh[:, 2, 2] = 1 + 2 * (y * y + z * z), 1 + 2 * (x * x + z * z), 1 + 2 * (x * x + y * y)
    Rh[:, 0, 1] = Rh[:, 1, 0] = 2 * (x * y + w * z)
    Rh[:, 0, 2] = Rh[:, 2, 0] = 2 * (x * z + w * y)
    Rh[:, 1, 2] = Rh[:, 2, 1] = 2 * (y * z + w * x)
    rh = np.einsum("nab,nb->na", Rh, np.abs(m[:, 3:6]))
    eh = np.abs(m[:, 0:3]) + np.abs(st[:, 0:3]) + rh
    lh = np.sqrt((eh * eh).sum(axis=1))
    av, ao = np.abs(st[:, 7:10]), np.abs(st[:, 10:13])
    uh = np.stack([av[:, 0] + ao[:, 1] * rh[:, 2] + ao[:, 2] * rh[:, 1],
                   av[:, 1] + ao[:, 2] * rh[:, 0] + ao[:, 0] * rh[:, 2],
                   av[:, 2] + ao[:, 0] * rh[:, 1] + ao[:, 1] * rh[:, 0]], axis=1)
    safe_l = np.where(on, l, 1.0)
    unh = (uh * eh).sum(axis=1) / safe_l
    Th = m[:, 7] * (lh + m[:, 6]) + m[:, 8] * unh
    Fh = Th[:, None] * eh / safe_l[:, None]
    Mh = np.stack([rh[:, 1] * Fh[:, 2] + rh[:, 2] * Fh[:, 1],
                   rh[:, 2] * Fh[:, 0] + rh[:, 0] * Fh[:, 2],
                   rh[:, 0] * Fh[:, 1] + rh[:, 1] * Fh[:, 0]], axis=1)
    return np.concatenate([Fh, Mh], axis=1) * on[:, None]


_fma32, _rsqrt_nr32 = br._fma32, br._rsqrt_nr32


def _fp32_terms(rec, state):
    """The header's operations in NumPy float32, in its order: (r, e, inv, x, T) - lists of (n,) float32 arrays."""
    f32 = np.float32
    m, st = np.asarray(rec, f32), np.asarray(state, f32)
    qx, qy, qz, qw = (st[:, 3 + i] for i in range(4))
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2
    wx, wy, wz = qw * x2, qw * y2, qw * z2
    R = [[f32(1) - (yy + zz), xy - wz, xz + wy], [xy + wz, f32(1) - (xx + zz), yz - wx], [xz - wy, yz + wx, f32(1) - (xx + yy)]]
    b = [m[:, 3], m[:, 4], m[:, 5]]
    r = [_fma32(R[i][2], b[2], _fma32(R[i][1], b[1], R[i][0] * b[0])) for i in range(3)]
    e = [(m[:, i] - st[:, i]) - r[i] for i in range(3)]
    l2 = _fma32(e[2], e[2], _fma32(e[1], e[1], e[0] * e[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = _rsqrt_nr32(l2)
        l = l2 * inv
        x = l - m[:, 6]
        ux = _fma32(st[:, 11], r[2], _fma32(-st[:, 12], r[1], st[:, 7]))
        uy = _fma32(st[:, 12], r[0], _fma32(-st[:, 10], r[2], st[:, 8]))
        uz = _fma32(st[:, 10], r[1], _fma32(-st[:, 11], r[0], st[:, 9]))
        un = _fma32(uz, e[2], _fma32(uy, e[1], ux * e[0])) * inv
        T = _fma32(m[:, 7], x, -(m[:, 8] * un))
        T = np.where(T > 0, T, f32(0))                             # max(0, .) that gives 0 for a NaN, as the hardware's does
    return r, e, inv, x, T


def taut_fp32(rec, state):
    """(n,) bool: the kernel's own decision - a line, and x > 0 in the fp32 operations include/hydro.h lists."""
    return has_line(np.asarray(rec, np.float32)) & (_fp32_terms(rec, state)[3] > 0)


def wrench_fp32_emulated(rec, state):
    """(n, 6) W by the operations of include/hydro.h in NumPy float32, in the header's order: what the kernel computes but for
    the seed of the reciprocal square root and the rare double rounding of _fma32."""
    f32 = np.float32
    r, e, inv, x, T = _fp32_terms(rec, state)
    on = has_line(np.asarray(rec, f32)) & (x > 0) & (T > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ti = T * inv
        F = [ti * e[i] for i in range(3)]
        M = [_fma32(r[1], F[2], -(r[2] * F[1])), _fma32(r[2], F[0], -(r[0] * F[2])), _fma32(r[0], F[1], -(r[1] * F[0]))]
    return np.where(on[:, None], np.stack(F + M, axis=1), f32(0)).astype(f32)


def closed_loop_moor(state, prev, params, rho, g, dt, steps, rec, bed=None, sea=None, step0=0, implicit=True, coeff_dtype="f32",
                     applied=None):
    """seabed_reference.closed_loop_bed with the fp64 line wrench added, bed and sea optional (`rec` None: no lines): per step
    hydro_oracle.step_wrench (on the fp32 state relative to `sea`, if there is one), + `applied` ((n, 6), world frame, may be
    None) + the fp64 bed wrench + the fp64 line wrench of the TRUE state, the sum rounded to fp32, integrator_oracle.integrate
    on the true state, the state rounded to fp32.  Returns per-step dicts: 'state' (after the step), 'input', 'wrench' (the
    sum), 'hydro' (the hydrodynamic wrench alone), 'line' (W), 'tension', 'taut'."""
    p = io._coeffs(params, coeff_dtype)
    st = np.asarray(state, dtype=np.float32)
    pv = np.asarray(prev, dtype=np.float32)
    n = len(st)
    out = []
    for k in range(steps):
        s_rel, pv_rel = st, pv
        if sea is not None:
            eta, u = sr.water(sea, st[:, 0], st[:, 1], st[:, 2], step0 + k, dt)
            s_rel, pv_rel = sr.relative(st, pv, eta.astype(np.float32), u.astype(np.float32))
        f, t, comps = ho.step_wrench(s_rel, pv_rel, p, rho, g, dt)
        hydro = np.concatenate([f, t], axis=1).astype(np.float64)
        total = hydro + (0.0 if applied is None else np.asarray(applied, np.float64))
        if bed is not None:
            total = total + br.wrench(bed, st, params)
        W = wrench(rec, st) if rec is not None else np.zeros((n, 6))
        T = tension(rec, st) if rec is not None else np.zeros(n)
        on = taut(rec, st) if rec is not None else np.zeros(n, bool)
        total = (total + W).astype(np.float32)
        kk = io.drag_jacobian(s_rel, p, comps, rho) if implicit else None
        new = io.integrate(st, total, p, g, dt, *(kk if kk is not None else (None, None)))
        out.append({"input": st, "wrench": total, "hydro": hydro, "line": W, "tension": T, "taut": on, "state": new.astype(np.float32)})
        pv, st = st[:, 7:13].copy(), out[-1]["state"]
    return out
