"""A sea state for the closed loop: a steady uniform current and up to eight regular deep-water wave components.

`SeaState` is what `ClosedLoopSim.set_sea` and `HydroEngine.set_sea` take.  The kernels evaluate the model of
include/hydro.h ("Sea state") in fp32 inside every physics step; `elevation` and `velocity` below restate it on the host
in fp64 NumPy - for plotting, for choosing a mooring, for checking a recorded trajectory against the surface it rode.

    eta(x, y, t) = sum_j a_j cos(kx_j x + ky_j y - omega_j t + phi_j)
    u(x, y, z_rel, t) = U + sum_j a_j omega_j exp(kappa_j min(z_rel, 0)) (kx_j / kappa_j cos th_j, ky_j / kappa_j cos th_j, sin th_j)

with z_rel the depth of the point below the local surface (z - eta) and kappa_j = |k_j|.  The library takes omega and k
as given; `regular` applies the deep-water dispersion relation omega^2 = g kappa.
"""
from __future__ import annotations

import math

import numpy as np

WAVES_MAX = 8


class SeaState:
    def __init__(self, current=(0.0, 0.0, 0.0)):
        cur = tuple(float(x) for x in current)
        if len(cur) != 3 or not all(math.isfinite(x) for x in cur):
            raise ValueError("current: expected three finite numbers (m/s, world frame)")
        self.current = cur
        self.waves: list[tuple[float, float, float, float, float]] = []     # (amplitude, kx, ky, omega, phase)

    def add_wave(self, amplitude: float, kx: float, ky: float, omega: float, phase: float = 0.0) -> "SeaState":
        """One regular component: amplitude (m, >= 0), wave vector (kx, ky) (rad/m), angular frequency (rad/s), phase (rad)."""
        w = (float(amplitude), float(kx), float(ky), float(omega), float(phase))
        if not all(math.isfinite(x) for x in w):
            raise ValueError("wave component: non-finite value")
        if w[0] < 0.0:
            raise ValueError("wave component: the amplitude must be >= 0")
        if w[0] != 0.0 and math.hypot(w[1], w[2]) == 0.0:
            raise ValueError("wave component: a wave with amplitude needs a wave vector")
        if len(self.waves) >= WAVES_MAX:
            raise ValueError(f"a sea has at most {WAVES_MAX} wave components")
        self.waves.append(w)
        return self

    @classmethod
    def regular(cls, height: float, period: float, heading_deg: float, phase: float = 0.0, g: float = 9.81,
                current=(0.0, 0.0, 0.0)) -> "SeaState":
        """One regular deep-water wave of crest-to-trough `height` (m) and `period` (s) travelling towards `heading_deg`
        (degrees from +x towards +y): omega = 2 pi / period, kappa = omega^2 / g."""
        if not period > 0.0 or not g > 0.0:
            raise ValueError("period and g must be > 0")
        omega = 2.0 * math.pi / period
        kappa = omega * omega / g
        h = math.radians(heading_deg)
        return cls(current).add_wave(0.5 * height, kappa * math.cos(h), kappa * math.sin(h), omega, phase)

    def _phases(self, x, y, t):
        x, y, t = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(t, np.float64)
        return [kx * x + ky * y - om * t + ph for _, kx, ky, om, ph in self.waves]

    def elevation(self, x, y, t) -> np.ndarray:
        """Surface elevation eta (m) at (x, y) and time t; the arguments broadcast."""
        x, y, t = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(t, np.float64))
        eta = np.zeros(x.shape, np.float64)
        for (a, *_), th in zip(self.waves, self._phases(x, y, t)):
            eta = eta + a * np.cos(th)
        return eta

    def velocity(self, x, y, z_rel, t) -> np.ndarray:
        """Water velocity (..., 3) (m/s, world frame) at (x, y), `z_rel` below the local surface (negative: submerged; at
        and above the surface the surface value), at time t; the arguments broadcast."""
        x, y, z, t = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z_rel, np.float64),
                                         np.asarray(t, np.float64))
        u = np.empty(x.shape + (3,), np.float64)
        u[...] = self.current
        zc = np.minimum(z, 0.0)
        for (a, kx, ky, om, _), th in zip(self.waves, self._phases(x, y, t)):
            kappa = math.hypot(kx, ky)
            if kappa == 0.0:
                continue
            e = a * om * np.exp(kappa * zc)
            u[..., 0] += e * (kx / kappa) * np.cos(th)
            u[..., 1] += e * (ky / kappa) * np.cos(th)
            u[..., 2] += e * np.sin(th)
        return u
