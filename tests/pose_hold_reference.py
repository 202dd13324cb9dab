"""The pose-hold law of hydro_step_fused_tiled_multi_ctl (include/hydro.h) restated in fp64 NumPy: the reference of
tests/test_pose_hold.py and tests/test_pose_hold_gpu.py.  No device, no library.

Control record per body, 17 fields:  p*(3) | q*(4, xyzw) | kp_lin(3) | kd_lin(3) | kp_ang | kd_ang | f_max | t_max
State per body, 13 fields:           p(3) | q(4, xyzw) | v(3) | omega(3)

    F = kp_lin * (p* - p) - kd_lin * v                    clamped to the norm f_max
    q_e = q* (x) conj(q), flipped to w >= 0;  T = kp_ang * 2 q_e.xyz - kd_ang * omega      clamped to the norm t_max
"""
import numpy as np

FIELDS = 17
P, Q, KP_LIN, KD_LIN, KP_ANG, KD_ANG, F_MAX, T_MAX = slice(0, 3), slice(3, 7), slice(7, 10), slice(10, 13), 13, 14, 15, 16


def record(n, position, orientation_xyzw, kp_lin=0.0, kd_lin=0.0, kp_ang=0.0, kd_ang=0.0, f_max=np.inf, t_max=np.inf):
    """(n, 17) float32 control record; every argument broadcasts over the bodies."""
    c = np.zeros((n, FIELDS), np.float32)
    c[:, P], c[:, Q] = position, orientation_xyzw
    c[:, KP_LIN], c[:, KD_LIN] = kp_lin, kd_lin
    c[:, KP_ANG], c[:, KD_ANG], c[:, F_MAX], c[:, T_MAX] = kp_ang, kd_ang, f_max, t_max
    return c


def error_quaternion(state, control):
    """q* (x) conj(q) as (n, 4) xyzw in fp64, BEFORE the sign flip (neither quaternion is normalised)."""
    s, c = np.asarray(state, np.float64), np.asarray(control, np.float64)
    tv, tw, qv, qw = c[:, 3:6], c[:, 6:7], s[:, 3:6], s[:, 6:7]
    w = tw * qw + np.sum(tv * qv, axis=1, keepdims=True)
    v = qw * tv - tw * qv + np.cross(qv, tv)
    return np.concatenate([v, w], axis=1)


def _clamp(x, top):
    """The header's comparison, literally: if (n2 > top * top) x = x * (top / sqrt(n2)).  A NaN `top` compares false and does not
    clamp; top = 0 gives a zero; a negative `top` acts where n2 > top^2 and turns the vector round (the record is the caller's)."""
    n2 = (x * x).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        acts = n2 > top * top
        k = np.where(acts, top / np.sqrt(n2), 1.0)
        return np.where(acts[:, None], x * k[:, None], x), acts


def unclamped(state, control):
    """(F, T) of the law before the clamps, (n, 3) each, fp64."""
    s, c = np.asarray(state, np.float64), np.asarray(control, np.float64)
    force = c[:, KP_LIN] * (c[:, P] - s[:, 0:3]) - c[:, KD_LIN] * s[:, 7:10]
    qe = error_quaternion(s, c)
    qe = np.where(qe[:, 3:4] < 0.0, -qe, qe)
    torque = c[:, KP_ANG, None] * 2.0 * qe[:, 0:3] - c[:, KD_ANG, None] * s[:, 10:13]
    return force, torque


def wrench(state, control):
    """(n, 6) fp64 [F | T] of the law, world frame, force at and torque about the body origin."""
    c = np.asarray(control, np.float64)
    force, torque = unclamped(state, control)
    return np.concatenate([_clamp(force, c[:, F_MAX])[0], _clamp(torque, c[:, T_MAX])[0]], axis=1)


def saturated(state, control):
    """(n,) bool pair: which bodies the force clamp and the torque clamp act on."""
    c = np.asarray(control, np.float64)
    force, torque = unclamped(state, control)
    return _clamp(force, c[:, F_MAX])[1], _clamp(torque, c[:, T_MAX])[1]


def term_magnitudes(state, control):
    """The sizes of the law's terms before they cancel - the yardstick of an fp32 evaluation's rounding error:
    per world axis |kp_lin e_p| + |kd_lin v| (n, 3), and kp_ang * 2 |q*| |q| + kd_ang |omega| (n,)."""
    s, c = np.asarray(state, np.float64), np.asarray(control, np.float64)
    lin = np.abs(c[:, KP_LIN] * (c[:, P] - s[:, 0:3])) + np.abs(c[:, KD_LIN] * s[:, 7:10])
    ang = (c[:, KP_ANG] * 2.0 * np.linalg.norm(c[:, Q], axis=1) * np.linalg.norm(s[:, 3:7], axis=1)
           + c[:, KD_ANG] * np.linalg.norm(s[:, 10:13], axis=1))
    return lin, ang
