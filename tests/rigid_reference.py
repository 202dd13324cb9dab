"""The rigid-body arithmetic the restatements of seabed, mooring line, tether and extremes share, each piece stated once: the
fp64 rotation and point kinematics, the term magnitudes an fp32 evaluation rounds against, and the fp32 operations of
include/hydro.h in NumPy float32, in the header's order.  What is specific to a model stays in its own *_reference module.
"""
import numpy as np


# ---- fp64 (or whatever dtype q has) ------------------------------------------------------------------------------------------------
def rot(q):
    """(n, 3, 3) matrices of the quaternions xyzw as given (non-unit included): 1 - 2(yy + zz), 2(xy - wz), ..."""
    x, y, z, w = (q[:, i] for i in range(4))
    R = np.empty((len(q), 3, 3), q.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - (y * (y + y) + z * (z + z)), x * (y + y) - w * (z + z), x * (z + z) + w * (y + y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = x * (y + y) + w * (z + z), 1 - (x * (x + x) + z * (z + z)), y * (z + z) - w * (x + x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = x * (z + z) - w * (y + y), y * (z + z) + w * (x + x), 1 - (x * (x + x) + y * (y + y))
    return R


# ---- term magnitudes: what fp32 rounds against ------------------------------------------------------------------------------------------
def rot_magnitudes(q):
    """R^ (n, 3, 3): the sums of the magnitudes of the terms of each entry of `rot` - diagonal 1 + |2yy| + |2zz|, off-diagonal
    |2xy| + |2wz| (symmetric)."""
    x, y, z, w = (np.abs(q[:, i]) for i in range(4))
    Rh = np.empty((len(q), 3, 3))
    Rh[:, 0, 0], Rh[:, 1, 1], Rh[:, 2, 2] = 1 + 2 * (y * y + z * z), 1 + 2 * (x * x + z * z), 1 + 2 * (x * x + y * y)
    Rh[:, 0, 1] = Rh[:, 1, 0] = 2 * (x * y + w * z)
    Rh[:, 0, 2] = Rh[:, 2, 0] = 2 * (x * z + w * y)
    Rh[:, 1, 2] = Rh[:, 2, 1] = 2 * (y * z + w * x)
    return Rh


def point_velocity_scale(v, omega, rh):
    """(n, 3) u^_x = |v_x| + |omega_y| r^_z + |omega_z| r^_y (cyclic): the scale of v + omega x r for an arm of magnitudes r^."""
    av, ao = np.abs(v), np.abs(omega)
    return np.stack([av[:, 0] + ao[:, 1] * rh[:, 2] + ao[:, 2] * rh[:, 1],
                     av[:, 1] + ao[:, 2] * rh[:, 0] + ao[:, 0] * rh[:, 2],
                     av[:, 2] + ao[:, 0] * rh[:, 1] + ao[:, 1] * rh[:, 0]], axis=1)


def cross_scale(rh, Fh):
    """r^ x^ F^ over the last axis, every product of the cross product counted positive."""
    return np.stack([rh[..., 1] * Fh[..., 2] + rh[..., 2] * Fh[..., 1],
                     rh[..., 2] * Fh[..., 0] + rh[..., 0] * Fh[..., 2],
                     rh[..., 0] * Fh[..., 1] + rh[..., 1] * Fh[..., 0]], axis=-1)


# ---- the header's fp32 operations ------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fma of fp32 operands: the product is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding that
    differs from the single one in about one case in 2^29)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def rsqrt_nr32(x):
    """rsqrt_nr with a correctly rounded seed in place of the hardware's (1 ulp)."""
    r = (1.0 / np.sqrt(x.astype(np.float64))).astype(np.float32)
    return fma32(fma32(-x * r, r, np.ones_like(x)), np.float32(0.5) * r, r)


def rot_fp32(q):
    """R[i][j], (n,) float32 each, of (n, 4) float32 quaternions: doubled components, products, one sum or difference each."""
    f32 = np.float32
    qx, qy, qz, qw = (q[:, i] for i in range(4))
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2
    wx, wy, wz = qw * x2, qw * y2, qw * z2
    return [[f32(1) - (yy + zz), xy - wz, xz + wy], [xy + wz, f32(1) - (xx + zz), yz - wx], [xz - wy, yz + wx, f32(1) - (xx + yy)]]


def point_velocity_fp32(state, r):
    """[u_x, u_y, u_z] of v + omega x r for an (n, 13) float32 state and an arm r (three (n,) float32): two fmas on v per axis."""
    st = state
    return [fma32(st[:, 11], r[2], fma32(-st[:, 12], r[1], st[:, 7])),
            fma32(st[:, 12], r[0], fma32(-st[:, 10], r[2], st[:, 8])),
            fma32(st[:, 10], r[1], fma32(-st[:, 11], r[0], st[:, 9]))]


def cross_fp32(r, F):
    """[M_x, M_y, M_z] of r x F: one product and one fma per axis."""
    return [fma32(r[1], F[2], -(r[2] * F[1])), fma32(r[2], F[0], -(r[0] * F[2])), fma32(r[0], F[1], -(r[1] * F[0]))]
