"""The seabed of hydro_step_fused_tiled_multi_bed (include/hydro.h, "Seabed") restated in fp64 NumPy: the reference of
tests/test_seabed.py and tests/test_seabed_gpu.py.  No device, no library, nothing of silver2_isaacsim_amd.seabed.

A bed is anything with `z`, `stiffness`, `damping`, `friction`, `slip_speed`, `friction_rate`.  Per corner
r_i = R (+-dx/2, +-dy/2, +-dz/2), i = 0 .. 7 with the signs of (i & 1, i & 2, i & 4), of a body [p | q | v | omega] of mass m:

    delta_i = z_b - (p_z + r_i,z)                       only delta_i > 0 contributes
    u_i     = v + omega x r_i
    N_i     = max(0, m (kappa delta_i - beta u_i,z))
    c_i     = min(mu N_i / sqrt(u_i,x^2 + u_i,y^2 + v_s^2), m gamma)
    F_i     = (-c_i u_i,x, -c_i u_i,y, N_i)             W = sum_i (F_i, r_i x F_i)

The bed sees the TRUE state; in a step W is added behind the applied wrench and the pose hold, in front of the integrator.

THE DECISION delta_i > 0 is where the model is discontinuous (a corner that arrives moving down meets the damper at full
strength), so a reference that decides in fp64 and a kernel that decides in fp32 may differ by a whole force at a corner that
stands within a rounding of the plane.  `touching_fp32` restates the kernel's decision in its own arithmetic - products,
additions and subtractions of fp32 numbers only, which NumPy's float32 reproduces exactly - and `wrench(..., touch=)` takes
it: the comparison then measures the arithmetic, not the tie.
"""
import numpy as np

from rigid_reference import cross_scale, fma32, point_velocity_fp32, point_velocity_scale, rot, rot_fp32, rot_magnitudes, rsqrt_nr32

ULP = 2.0 ** -24
PROBE_BOUND = 4.0            # units of 2^-24 of wrench_scales: the bound of hydro_seabed_wrench (tests/test_seabed_gpu.py's docstring)
SIGNS = [(-1.0 if not i & 1 else 1.0, -1.0 if not i & 2 else 1.0, -1.0 if not i & 4 else 1.0) for i in range(8)]


def _consts(bed):
    return tuple(float(getattr(bed, k)) for k in ("z", "stiffness", "damping", "friction", "slip_speed", "friction_rate"))


def corners(state, params):
    """(n, 8, 3) offsets of the corners from the body origin, world frame, fp64."""
    st, pr = np.asarray(state, np.float64), np.asarray(params, np.float64)
    R = rot(st[:, 3:7])
    out = np.empty((len(st), 8, 3))
    for i, (sx, sy, sz) in enumerate(SIGNS):
        local = np.stack([sx * 0.5 * pr[:, 0], sy * 0.5 * pr[:, 1], sz * 0.5 * pr[:, 2]], axis=1)
        out[:, i, :] = np.einsum("nab,nb->na", R, local)
    return out


def penetration(bed, state, params):
    """(n, 8) delta_i in fp64 (positive: the corner is below the plane)."""
    st = np.asarray(state, np.float64)
    return _consts(bed)[0] - (st[:, None, 2] + corners(state, params)[:, :, 2])


def touching_fp32(bed, state, params):
    """(n, 8) bool: the kernel's own decision delta_i > 0, in the fp32 operations include/hydro.h lists (no fused operation
    among them: R from products and sums, A_z = 0.5 (R_20 dx) ..., r_z = (s_x A_z + s_y B_z) + s_z C_z, z_b - (p_z + r_z))."""
    st, pr = np.asarray(state, np.float32), np.asarray(params, np.float32)
    r20, r21, r22 = rot_fp32(st[:, 3:7])[2]
    az, bz, cz = np.float32(0.5) * (r20 * pr[:, 0]), np.float32(0.5) * (r21 * pr[:, 1]), np.float32(0.5) * (r22 * pr[:, 2])
    zb = np.float32(_consts(bed)[0])
    out = np.empty((len(st), 8), bool)
    for i, (sx, sy, sz) in enumerate(SIGNS):
        rz = (np.float32(sx) * az + np.float32(sy) * bz) + np.float32(sz) * cz
        out[:, i] = zb - (st[:, 2] + rz) > 0
    return out


def _corner_terms(bed, state, params, touch):
    st, pr = np.asarray(state, np.float64), np.asarray(params, np.float64)
    zb, kappa, beta, mu, vs, gamma = _consts(bed)
    m = pr[:, 10]
    r = corners(state, params)
    delta = zb - (st[:, None, 2] + r[:, :, 2])
    on = delta > 0 if touch is None else np.asarray(touch, bool)
    v, om = st[:, None, 7:10], st[:, None, 10:13]
    u = v + np.cross(np.broadcast_to(om, r.shape), r)
    N = np.where(on, np.maximum(0.0, m[:, None] * (kappa * delta - beta * u[:, :, 2])), 0.0)
    c = np.minimum(mu * N / np.sqrt(u[:, :, 0] ** 2 + u[:, :, 1] ** 2 + vs * vs), (m * gamma)[:, None])
    F = np.stack([-c * u[:, :, 0], -c * u[:, :, 1], N], axis=2)
    return r, delta, u, F, on


def wrench(bed, state, params, touch=None):
    """(n, 6) W in fp64; `touch` (n, 8): which corners contribute, default delta_i > 0 decided in fp64."""
    r, _, _, F, _ = _corner_terms(bed, state, params, touch)
    return np.concatenate([F.sum(axis=1), np.cross(r, F).sum(axis=1)], axis=1)


def corner_count(bed, state, params, touch=None):
    """(n,) corners below the plane."""
    return _corner_terms(bed, state, params, touch)[4].sum(axis=1)


def wrench_scales(bed, state, params, touch=None):
    """What an fp32 evaluation of W rounds against, per body and component (n, 6): the sum of the magnitudes of the terms that
    form it.  With R^ the matrix of term magnitudes of R (diagonal 1 + |2yy| + |2zz|, off-diagonal |2xy| + |2wz|) and
    r^_k = sum_j R^_kj d_j / 2 (the same for all corners):
        delta^ = |z_b| + |p_z| + r^_z             u^_x = |v_x| + |omega_y| r^_z + |omega_z| r^_y   (cyclic)
        N^     = m (kappa delta^ + beta u^_z)      of a contributing corner
        c^     = mu N^ / sqrt(.) where the friction is below its cap (the fp64 root; N^, not N: the rounding of delta
                 reaches c through N whatever is left of N after the cancellation), m gamma where the cap holds
        F^     = (c^ u^_x, c^ u^_y, N^)
        W^_F   = sum_i F^                          W^_T = sum_i r^ x^ F^  with every product of the cross product counted positive"""
    st, pr = np.asarray(state, np.float64), np.asarray(params, np.float64)
    zb, kappa, beta, mu, vs, gamma = _consts(bed)
    m = pr[:, 10]
    _, _, u, F, on = _corner_terms(bed, state, params, touch)
    rh = np.einsum("nab,nb->na", rot_magnitudes(st[:, 3:7]), 0.5 * pr[:, 0:3])
    dh = abs(zb) + np.abs(st[:, 2]) + rh[:, 2]
    uh = point_velocity_scale(st[:, 7:10], st[:, 10:13], rh)
    Nh = m * (kappa * dh + beta * uh[:, 2])
    root = np.sqrt(u[:, :, 0] ** 2 + u[:, :, 1] ** 2 + vs * vs)                          # (n, 8)
    capped = mu * F[:, :, 2] / root >= (m * gamma)[:, None]
    ch = np.where(capped, (m * gamma)[:, None], mu * Nh[:, None] / root)
    Fh = np.stack([ch * uh[:, None, 0], ch * uh[:, None, 1], np.broadcast_to(Nh[:, None], ch.shape)], axis=2) * on[:, :, None]
    return np.concatenate([Fh.sum(axis=1), cross_scale(rh[:, None, :], Fh).sum(axis=1)], axis=1)


def wrench_fp32_emulated(bed, state, params):
    """(n, 6) W by the operations of include/hydro.h in NumPy float32, corner by corner in the header's order: what the
    kernel computes but for the seed of the reciprocal square root and the rare double rounding of fma32."""
    f32 = np.float32
    st, pr = np.asarray(state, f32), np.asarray(params, f32)
    zb, ka, be, mu, vs, ga = (f32(v) for v in _consts(bed))
    R = rot_fp32(st[:, 3:7])
    A, B, C = ([f32(0.5) * (R[k][j] * pr[:, j]) for k in range(3)] for j in range(3))
    m, n = pr[:, 10], len(st)
    W = [np.zeros(n, f32) for _ in range(6)]
    kav, vsv = np.full(n, ka, f32), np.full(n, vs, f32)
    for sx, sy, sz in SIGNS:
        r = [(f32(sx) * A[k] + f32(sy) * B[k]) + f32(sz) * C[k] for k in range(3)]
        delta = zb - (st[:, 2] + r[2])
        ux, uy, uz = point_velocity_fp32(st, r)
        a = np.maximum(f32(0), fma32(kav, delta, -(be * uz)))
        N = m * a
        c = m * np.minimum((mu * a) * rsqrt_nr32(fma32(vsv, vsv, fma32(uy, uy, ux * ux))), ga)
        tx, ty = c * ux, c * uy
        new = [W[0] - tx, W[1] - ty, W[2] + N, fma32(r[1], N, fma32(r[2], ty, W[3])),
               fma32(-r[2], tx, fma32(-r[0], N, W[4])), fma32(r[1], tx, fma32(-r[0], ty, W[5]))]
        W = [np.where(delta > 0, nw, w) for nw, w in zip(new, W)]
    return np.stack(W, axis=1)
