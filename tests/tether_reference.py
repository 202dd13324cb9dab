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

from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io

import mooring_reference as mr
import sea_reference as sr
import seabed_reference as br

ULP = 2.0 ** -24
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
    r = np.einsum("nab,nb->na", br._rot(st[:, 3:7]), t[:, 0:3])
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
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where((T > 0)[:, None], (T / l)[:, None] * e, 0.0)
    return np.concatenate([F, np.cross(r, F)], axis=1)


def _magnitudes(rec, state):
    """(r^, P^, U^) per body: the sums of the magnitudes of the terms that form the arm, the fairlead and its velocity."""
    t, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    x, y, z, w = (np.abs(st[:, 3 + i]) for i in range(4))
    Rh = np.empty((len(st), 3, 3))
    Rh[:, 0, 0], Rh[:, 1, 1], Rh[:, 2, 2] = 1 + 2 * (y * y + z * z), 1 + 2 * (x * x + z * z), 1 + 2 * (x * x + y * y)
    Rh[:, 0, 1] = Rh[:, 1, 0] = 2 * (x * y + w * z)
    Rh[:, 0, 2] = Rh[:, 2, 0] = 2 * (x * z + w * y)
    Rh[:, 1, 2] = Rh[:, 2, 1] = 2 * (y * z + w * x)
    rh = np.einsum("nab,nb->na", Rh, np.abs(t[:, 0:3]))
    Ph = np.abs(st[:, 0:3]) + rh
    av, ao = np.abs(st[:, 7:10]), np.abs(st[:, 10:13])
    Uh = np.stack([av[:, 0] + ao[:, 1] * rh[:, 2] + ao[:, 2] * rh[:, 1],
                   av[:, 1] + ao[:, 2] * rh[:, 0] + ao[:, 0] * rh[:, 2],
                   av[:, 2] + ao[:, 0] * rh[:, 1] + ao[:, 1] * rh[:, 0]], axis=1)
    return rh, Ph, Uh


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
    Mh = np.stack([rh[:, 1] * Fh[:, 2] + rh[:, 2] * Fh[:, 1],
                   rh[:, 2] * Fh[:, 0] + rh[:, 0] * Fh[:, 2],
                   rh[:, 0] * Fh[:, 1] + rh[:, 1] * Fh[:, 0]], axis=1)
    return np.concatenate([Fh, Mh], axis=1) * on[:, None]


def tension_scale(rec, state, taut=None, contributing=None):
    """(n,) T^ of wrench_scales: what the tension rounds against; 0 where the tether adds nothing."""
    t = np.asarray(rec, np.float64)
    _, _, l, _, _, _ = geometry(rec, state)
    on = tension(rec, state, taut) > 0 if contributing is None else np.asarray(contributing, bool)
    _, Ph, Uh = _magnitudes(rec, state)
    eh, dUh = _from_partner(rec, Ph) + Ph, _from_partner(rec, Uh) + Uh
    safe_l = np.where(on & (l > 0), l, 1.0)
    return (t[:, 4] * (np.sqrt((eh * eh).sum(axis=1)) + t[:, 3]) + t[:, 5] * (dUh * eh).sum(axis=1) / safe_l) * on


_fma32, _rsqrt_nr32 = br._fma32, br._rsqrt_nr32


def _fp32_terms(rec, state):
    """The header's operations in NumPy float32, in its order: (r, e, inv, x, T) - lists of (n,) float32 arrays."""
    f32 = np.float32
    t, st = np.asarray(rec, f32), np.asarray(state, f32)
    qx, qy, qz, qw = (st[:, 3 + i] for i in range(4))
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2
    wx, wy, wz = qw * x2, qw * y2, qw * z2
    R = [[f32(1) - (yy + zz), xy - wz, xz + wy], [xy + wz, f32(1) - (xx + zz), yz - wx], [xz - wy, yz + wx, f32(1) - (xx + yy)]]
    b = [t[:, 0], t[:, 1], t[:, 2]]
    r = [_fma32(R[i][2], b[2], _fma32(R[i][1], b[1], R[i][0] * b[0])) for i in range(3)]
    P = [st[:, i] + r[i] for i in range(3)]
    U = [_fma32(st[:, 11], r[2], _fma32(-st[:, 12], r[1], st[:, 7])),
         _fma32(st[:, 12], r[0], _fma32(-st[:, 10], r[2], st[:, 8])),
         _fma32(st[:, 10], r[1], _fma32(-st[:, 11], r[0], st[:, 9]))]
    e = [_from_partner(rec, P[i]) - P[i] for i in range(3)]
    dU = [_from_partner(rec, U[i]) - U[i] for i in range(3)]
    l2 = _fma32(e[2], e[2], _fma32(e[1], e[1], e[0] * e[0]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = _rsqrt_nr32(l2)
        l = l2 * inv
        x = l - t[:, 3]
        rate = _fma32(dU[2], e[2], _fma32(dU[1], e[1], dU[0] * e[0])) * inv
        T = _fma32(t[:, 4], x, t[:, 5] * rate)
        T = np.where(T > 0, T, f32(0))                             # max(0, .) that gives 0 for a NaN, as the hardware's does
    return r, e, inv, x, T


def taut_fp32(rec, state):
    """(n,) bool: the kernel's own decision - a tether, and x > 0 in the fp32 operations include/hydro.h lists."""
    return has_tether(np.asarray(rec, np.float32)) & (_fp32_terms(rec, state)[3] > 0)


def wrench_fp32_emulated(rec, state, with_tension=False):
    """(n, 6) W by the operations of include/hydro.h in NumPy float32, in the header's order: what the kernel computes but for
    the seed of the reciprocal square root and the rare double rounding of _fma32.  with_tension: (W, T), T (n,) float32."""
    f32 = np.float32
    r, e, inv, x, T = _fp32_terms(rec, state)
    on = has_tether(np.asarray(rec, f32)) & (x > 0) & (T > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ti = T * inv
        F = [ti * e[i] for i in range(3)]
        M = [_fma32(r[1], F[2], -(r[2] * F[1])), _fma32(r[2], F[0], -(r[0] * F[2])), _fma32(r[0], F[1], -(r[1] * F[0]))]
    W = np.where(on[:, None], np.stack(F + M, axis=1), f32(0)).astype(f32)
    return (W, np.where(on, T, f32(0)).astype(f32)) if with_tension else W


def closed_loop_teth(state, prev, params, rho, g, dt, steps, rec, moor=None, bed=None, sea=None, step0=0, implicit=True, coeff_dtype="f32",
                     applied=None, hydro=True):
    """mooring_reference.closed_loop_moor with the fp64 tether wrench added behind the mooring line's (`rec` None: no tethers;
    `moor`: an (n, 9) mooring record or None): per step hydro_oracle.step_wrench (on the fp32 state relative to `sea`, if there
    is one), + `applied` + the fp64 bed wrench + the fp64 mooring wrench + the fp64 tether wrench of the TRUE state, the sum
    rounded to fp32, integrator_oracle.integrate on the true state, the state rounded to fp32.  hydro=False: a scene in which
    only the tether acts - no hydrodynamic wrench, and the caller passes g = 0.  Returns per-step dicts: 'state' (after the step),
    'input', 'wrench' (the sum), 'hydro', 'line' (the tether's W), 'tension', 'taut'."""
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
        comps = None
        if hydro:
            f, t, comps = ho.step_wrench(s_rel, pv_rel, p, rho, g, dt)
            h = np.concatenate([f, t], axis=1).astype(np.float64)
        else:
            h = np.zeros((n, 6))
        total = h + (0.0 if applied is None else np.asarray(applied, np.float64))
        if bed is not None:
            total = total + br.wrench(bed, st, params)
        if moor is not None:
            total = total + mr.wrench(moor, st)
        W = wrench(rec, st) if rec is not None else np.zeros((n, 6))
        T = tension(rec, st) if rec is not None else np.zeros(n)
        on = taut(rec, st) if rec is not None else np.zeros(n, bool)
        total = (total + W).astype(np.float32)
        kk = io.drag_jacobian(s_rel, p, comps, rho) if (implicit and hydro) else None
        new = io.integrate(st, total, p, g, dt, *(kk if kk is not None else (None, None)))
        out.append({"input": st, "wrench": total, "hydro": h, "line": W, "tension": T, "taut": on, "state": new.astype(np.float32)})
        pv, st = st[:, 7:13].copy(), out[-1]["state"]
    return out
