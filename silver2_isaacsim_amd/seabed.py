"""A seabed for the closed loop: the horizontal plane z = z_b and a penalty contact at the eight corners of each body's box.

`Seabed` is what `ClosedLoopSim.set_seabed` and `HydroEngine.set_seabed` take.  The kernels evaluate the model of
include/hydro.h ("Seabed") in fp32 inside every physics step; `Seabed.wrench` restates it on the host in fp64 NumPy - for
checking a recorded trajectory, for sizing a thruster against the friction, for choosing the constants.

The five contact constants are mass-normalised (the force is the constant times the body's mass).  For the corners
r_i = R (+-dx/2, +-dy/2, +-dz/2) of a body with position p, velocity v, angular velocity omega and mass m:

    delta_i = z_b - (p_z + r_i,z)                       only delta_i > 0 contributes
    u_i     = v + omega x r_i
    N_i     = max(0, m (stiffness delta_i - damping u_i,z))
    c_i     = min(friction N_i / sqrt(u_i,x^2 + u_i,y^2 + slip_speed^2), m friction_rate)
    F_i     = (-c_i u_i,x, -c_i u_i,y, N_i)
    W       = sum_i (F_i, r_i x F_i)

A box at rest on four corners stands g (1 - rho / rho_body) / (4 stiffness) below z_b (`rest_depth`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np


def rotation_matrices(q_xyzw: np.ndarray) -> np.ndarray:
    """(n, 3, 3) body -> world matrices of the quaternions as given (non-unit included), in the form the kernels build them."""
    x, y, z, w = (np.asarray(q_xyzw, np.float64)[:, i] for i in range(4))
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2
    sx, sy, sz = w * x2, w * y2, w * z2
    return np.stack([np.stack([1.0 - (yy + zz), xy - sz, xz + sy], -1),
                     np.stack([xy + sz, 1.0 - (xx + zz), yz - sx], -1),
                     np.stack([xz - sy, yz + sx, 1.0 - (xx + yy)], -1)], -2)


# the corners in the kernel's order: i = 0 .. 7, signs (i & 1, i & 2, i & 4) -> (x, y, z)
CORNER_SIGNS = np.array([[1.0 if i & 1 else -1.0, 1.0 if i & 2 else -1.0, 1.0 if i & 4 else -1.0] for i in range(8)])


@dataclass(frozen=True)
class Seabed:
    z: float                    # height of the plane (m)
    stiffness: float            # kappa, 1/s^2
    damping: float              # beta, 1/s
    friction: float = 0.5       # mu
    slip_speed: float = 0.01    # v_s, m/s
    friction_rate: float = 0.0  # gamma, 1/s

    def __post_init__(self):
        v = (self.z, self.stiffness, self.damping, self.friction, self.slip_speed, self.friction_rate)
        if not all(math.isfinite(float(x)) for x in v):
            raise ValueError("seabed: non-finite value")
        if self.stiffness < 0 or self.damping < 0 or self.friction < 0 or self.friction_rate < 0:
            raise ValueError("seabed: stiffness, damping, friction and friction_rate must be >= 0")
        if not self.slip_speed > 0:
            raise ValueError("seabed: slip_speed must be > 0")

    @classmethod
    def for_step(cls, z: float, dt: float, friction: float = 0.5, slip_speed: float = 0.01) -> "Seabed":
        """The constants that are stable for a physics step `dt`: stiffness (0.2 / dt)^2, damping and friction_rate 0.04 / dt -
        per corner kappa dt^2 <= 0.04 and beta dt, gamma dt <= 0.04 (include/hydro.h)."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        return cls(float(z), (0.2 / dt) ** 2, 0.04 / dt, float(friction), float(slip_speed), 0.04 / dt)

    def rest_depth(self, density_ratio: float, g: float = 9.81) -> float:
        """How far below z_b the four lower corners of a box of rho_body / rho = `density_ratio` stand at rest (m, >= 0)."""
        return g * (1.0 - 1.0 / density_ratio) / (4.0 * self.stiffness)

    def corners(self, state, params) -> np.ndarray:
        """(n, 8, 3) corner offsets r_i from the body origin, world frame."""
        state, params = np.asarray(state, np.float64), np.asarray(params, np.float64)
        R = rotation_matrices(state[:, 3:7])
        local = CORNER_SIGNS[None, :, :] * (0.5 * params[:, None, 0:3])
        return np.einsum("nkj,nij->nik", R, local)

    def wrench(self, state, params) -> np.ndarray:
        """(n, 6) contact wrench [F | T about the body origin], world frame, of (n, 13) states [p | q xyzw | v | omega] and
        (n, 11) parameters (dimensions first, mass last), in fp64."""
        state, params = np.asarray(state, np.float64), np.asarray(params, np.float64)
        m = params[:, 10][:, None]
        r = self.corners(state, params)
        delta = self.z - (state[:, None, 2] + r[..., 2])
        u = state[:, None, 7:10] + np.cross(state[:, None, 10:13], r)
        touch = delta > 0.0
        N = np.where(touch, np.maximum(0.0, m * (self.stiffness * delta - self.damping * u[..., 2])), 0.0)
        c = np.minimum(self.friction * N / np.sqrt(u[..., 0] ** 2 + u[..., 1] ** 2 + self.slip_speed ** 2), m * self.friction_rate)
        F = np.stack([-c * u[..., 0], -c * u[..., 1], N], -1)
        return np.concatenate([F.sum(1), np.cross(r, F).sum(1)], -1)
