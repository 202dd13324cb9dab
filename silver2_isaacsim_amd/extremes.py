"""Per-body extremes of a closed-loop run: the box a body stayed in, its largest speed and its largest line tension.

The kernels of `HydroEngine.step_fused_tiled_multi_ext` keep, per body, a record of eight floats (include/hydro.h,
"Extremes") and update it after EVERY physics step, inside the launch - a design-load study of a million moored bodies over
a long storm reads eight numbers per body, not a trajectory:

    x_min x_max | y_min y_max | z_min z_max | speed2_max | tension_max

After step k the sample is the state the step produced (x, y, z, and speed2 = fma(v_z, v_z, fma(v_y, v_y, v_x * v_x)) in
fp32) and the tension T the mooring line formed in that step (+0 where the line adds nothing).  The update is a
compare-and-select, `m = x if x < m else m`, `M = x if x > M else M`: a NaN sample never enters, a NaN accumulator stays,
an equal value (-0 against +0 included) leaves the accumulator's bits.  The record accumulates over launches until it is
reset - to the empty record [+inf, -inf, +inf, -inf, +inf, -inf, +0, +0], or seeded from a state so that a run's initial
state counts.

`Extremes.fold` restates the update on the host, bit for bit; an `Extremes` object is the view
`ClosedLoopSim.track_extremes()` returns over the tiled device record.  Not provided: means, variances, the step at which
an extreme occurred, extremes of the wrench.
"""
from __future__ import annotations

import numpy as np

FIELDS = 8
NAMES = ("x_min", "x_max", "y_min", "y_max", "z_min", "z_max", "speed2_max", "tension_max")
X_MIN, X_MAX, Y_MIN, Y_MAX, Z_MIN, Z_MAX, SPEED2_MAX, TENSION_MAX = range(FIELDS)
INDEX = dict(zip(NAMES, range(FIELDS)))
EMPTY = np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32)


def fma32(a, b, c) -> np.ndarray:
    """fma of fp32 operands, rounded ONCE to fp32, elementwise.  The product of two fp32 values is exact in fp64; the sum is
    rounded to fp64 TO ODD (the error of the fp64 addition, from a two-sum, says whether it was exact and which way it went),
    and a value rounded to odd at 53 bits rounds to 24 bits as the exact one does."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        nudge = np.isfinite(s) & (err != 0.0) & even
        s = np.where(nudge, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def speed2(v) -> np.ndarray:
    """The kernel's squared speed of (., 3) fp32 velocities: fma(v_z, v_z, fma(v_y, v_y, v_x * v_x)), each rounded once."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return fma32(v[..., 2], v[..., 2], fma32(v[..., 1], v[..., 1], v[..., 0] * v[..., 0]))


def seed_of(state) -> np.ndarray:
    """(n, 8) record of the one sample `state` (n, 13): min = max = p, speed2 of its v, tension +0."""
    s = np.asarray(state, np.float32)
    rec = np.zeros((s.shape[0], FIELDS), np.float32)
    for a in range(3):
        rec[:, 2 * a] = rec[:, 2 * a + 1] = s[:, a]
    rec[:, SPEED2_MAX] = speed2(s[:, 7:10])
    return rec


class Extremes:
    """View over the tiled (tiles, 8, 64) device record of a `ClosedLoopSim` (`sim.track_extremes()`): `buffer` is the
    tensor the kernels read and write - its address never changes; every reader waits for the step stream first."""

    def __init__(self, sim, buffer):
        self._sim = sim
        self.buffer = buffer
        self.n = sim.n

    @staticmethod
    def empty(n: int) -> np.ndarray:
        """(n, 8) empty record: [+inf, -inf, +inf, -inf, +inf, -inf, +0, +0] per body."""
        return np.tile(EMPTY, (int(n), 1))

    @staticmethod
    def fold(states, tensions, seed=None) -> np.ndarray:
        """The host restatement: the (n, 8) fp32 record after the samples `states` (rows, n, 13) and `tensions` (rows, n)
        have entered, row by row, a record that starts as `seed` (n, 8; the empty record if None) - the kernel's
        compare-and-select and its formula for speed2, bit for bit."""
        states = np.asarray(states, np.float32)
        tensions = np.asarray(tensions, np.float32)
        if states.ndim != 3 or states.shape[2] != 13 or tensions.shape != states.shape[:2]:
            raise ValueError("fold: states must be (rows, n, 13) and tensions (rows, n)")
        n = states.shape[1]
        rec = Extremes.empty(n) if seed is None else np.array(seed, np.float32, copy=True)
        if rec.shape != (n, FIELDS):
            raise ValueError(f"fold: seed must be ({n}, {FIELDS})")
        with np.errstate(invalid="ignore"):
            for s, T in zip(states, tensions):
                for a in range(3):
                    lo, hi = rec[:, 2 * a], rec[:, 2 * a + 1]
                    rec[:, 2 * a] = np.where(s[:, a] < lo, s[:, a], lo)
                    rec[:, 2 * a + 1] = np.where(s[:, a] > hi, s[:, a], hi)
                for f, x in ((SPEED2_MAX, speed2(s[:, 7:10])), (TENSION_MAX, T)):
                    rec[:, f] = np.where(x > rec[:, f], x, rec[:, f])
        return rec

    def bodies(self) -> np.ndarray:
        """(n, 8) host copy of the record, one row per body, fields in the order of `NAMES`."""
        from . import scenes
        self._sim.synchronize()
        return scenes.from_tiled(self.buffer.cpu().numpy(), self.n)

    def field(self, name: str) -> np.ndarray:
        return self.bodies()[:, INDEX[name]]

    def x_min(self) -> np.ndarray: return self.field("x_min")
    def x_max(self) -> np.ndarray: return self.field("x_max")
    def y_min(self) -> np.ndarray: return self.field("y_min")
    def y_max(self) -> np.ndarray: return self.field("y_max")
    def z_min(self) -> np.ndarray: return self.field("z_min")
    def z_max(self) -> np.ndarray: return self.field("z_max")
    def speed2_max(self) -> np.ndarray: return self.field("speed2_max")
    def tension_max(self) -> np.ndarray: return self.field("tension_max")

    def speed_max(self) -> np.ndarray:
        """(n,) largest speed, m/s: the square root of speed2_max."""
        return np.sqrt(self.speed2_max().astype(np.float64))

    def excursion(self, origin_xy, record=None) -> np.ndarray:
        """(n,) watch circle: the largest horizontal distance from `origin_xy` ((2,) or (n, 2)) of the corners of the box
        [x_min, x_max] x [y_min, y_max] - an upper bound of the distance the body reached (the box is reached side by side,
        not necessarily at a corner).  NaN for a body whose box is empty."""
        return excursion(self.bodies() if record is None else record, origin_xy)

    def reset(self, from_state: bool = True) -> None:
        """Start over, on the sim's stream: from the sim's current state (it then counts as the first sample) or, with
        from_state=False, from the empty record."""
        import torch
        sim = self._sim
        with torch.cuda.stream(sim.stream):
            sim.engine.extremes_reset(self.buffer, sim.n, sim.cur if from_state else None)


def excursion(record, origin_xy) -> np.ndarray:
    """`Extremes.excursion` of an (n, 8) host record."""
    rec = np.asarray(record, np.float64)
    o = np.broadcast_to(np.asarray(origin_xy, np.float64), (rec.shape[0], 2))
    with np.errstate(invalid="ignore"):
        dx = np.maximum(np.abs(rec[:, X_MIN] - o[:, 0]), np.abs(rec[:, X_MAX] - o[:, 0]))
        dy = np.maximum(np.abs(rec[:, Y_MIN] - o[:, 1]), np.abs(rec[:, Y_MAX] - o[:, 1]))
        d = np.hypot(dx, dy)
    return np.where(np.isfinite(d), d, np.nan)
