"""Mooring lines for the closed loop: per body one tension-only line from an anchor in the world to a fairlead on the body.

`Mooring` builds and validates the (n, 9) record `ClosedLoopSim.set_mooring` tiles onto the device and
`HydroEngine.step_fused_tiled_multi_moor` / `mooring_wrench` take.  The kernels evaluate the model of include/hydro.h
("Mooring") in fp32 inside every physics step; `Mooring.wrench` restates it on the host in fp64 NumPy - for checking a
recorded trajectory, for sizing a line.

For a body with position p, rotation R, velocity v, angular velocity omega, and a line with anchor a (world), fairlead b
(body), unstretched length L0, stiffness k and damping c:

    r  = R b                            the fairlead's arm
    e  = a - p - r                      fairlead -> anchor,  l = |e|
    x  = l - L0                         the line is taut only if x > 0
    un = (v + omega x r) . e / l        > 0: the fairlead approaches the anchor
    T  = max(0, k x - c un)             a line cannot push
    F  = T e / l,    W = (F, r x F)

A body has a line if k > 0 or c > 0.  This is an explicit spring: k dt^2 / m and c dt / m must stay at or below 0.04
(`STABLE`); `Mooring.for_body(mass, dt)` gives k = 0.004 m / dt^2 and c = 0.02 m / dt, and `check_stable` refuses a record
that breaks the rule.  Not modelled: the line's mass and sag, drag on the line, the line on the bed, a line between two
bodies (`tether`).

`MooringSpread` puts a body on up to `LAYERS_MAX` = 4 such lines - the three- or four-line spread that keeps a floating body
on station where one line gives it a watch circle.  It is one `Mooring` per line ("layer"), so every per-line rule is the one
above; the wrenches add up, and the stability rule holds for the SUMS of k and of c over a body's lines, which may all be taut
at once.  Not modelled: more than four lines per body; a peak-tension record per line (the extremes record keeps the largest
tension of any of the body's lines).
"""
from __future__ import annotations

import numpy as np

from .seabed import rotation_matrices

FIELDS = 9                      # a(3) | b(3) | L0 | k | c
STABLE = 0.04                   # the bound on k dt^2 / m and on c dt / m
DEFAULT_K, DEFAULT_C = 0.004, 0.02
LAYERS_MAX = 4                  # lines per body in a spread (HYDRO_MOOR_LAYERS_MAX)


class Mooring:
    def __init__(self, anchor, fairlead=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, n: int | None = None):
        """`anchor` (n, 3) world, `fairlead` (n, 3) body frame, `length`, `stiffness`, `damping` (n,) - each broadcast to n
        bodies (`n`: from the anchor's rows if not given).  ValueError for a non-finite value or a negative length,
        stiffness or damping."""
        anchor = np.asarray(anchor, np.float64)
        if anchor.ndim > 2 or anchor.shape[-1:] != (3,):
            raise ValueError("mooring: anchor must be (3,) or (n, 3)")
        if n is None:
            n = anchor.shape[0] if anchor.ndim == 2 else 1
        fairlead = np.asarray(fairlead, np.float64)
        if fairlead.ndim > 2 or fairlead.shape[-1:] != (3,):
            raise ValueError("mooring: fairlead must be (3,) or (n, 3)")
        rec = np.empty((int(n), FIELDS), np.float64)
        try:
            rec[:, 0:3] = anchor
            rec[:, 3:6] = fairlead
            rec[:, 6] = np.asarray(length, np.float64)
            rec[:, 7] = np.asarray(stiffness, np.float64)
            rec[:, 8] = np.asarray(damping, np.float64)
        except ValueError as e:
            raise ValueError(f"mooring: a field does not fit {int(n)} bodies ({e})") from None
        if not np.isfinite(rec).all():
            raise ValueError("mooring: non-finite value")
        if (rec[:, 6:9] < 0.0).any():
            raise ValueError("mooring: length, stiffness and damping must be >= 0")
        self.record = rec

    @property
    def n(self) -> int:
        return self.record.shape[0]

    @staticmethod
    def for_body(mass, dt: float):
        """The default (stiffness, damping) of a line on a body of `mass` stepped with `dt`: k = 0.004 m / dt^2,
        c = 0.02 m / dt - a tenth and a half of the stability bound (include/hydro.h)."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        mass = np.asarray(mass, np.float64)
        if not (np.isfinite(mass).all() and (mass > 0.0).all()):
            raise ValueError("mass must be finite and > 0")
        k, c = DEFAULT_K * mass / dt ** 2, DEFAULT_C * mass / dt
        return (float(k), float(c)) if mass.ndim == 0 else (k, c)

    def check_stable(self, mass, dt: float) -> None:
        """ValueError if a line breaks the rule of thumb k dt^2 / m <= 0.04, c dt / m <= 0.04 for bodies of `mass`."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        mass = np.broadcast_to(np.asarray(mass, np.float64), (self.n,))
        tol = 1.0 + 1e-9
        ks, cs = self.record[:, 7] * dt ** 2 / mass, self.record[:, 8] * dt / mass
        if (ks > STABLE * tol).any() or (cs > STABLE * tol).any():
            i = int(np.argmax(np.maximum(ks, cs)))
            raise ValueError(f"mooring: body {i} has k dt^2 / m = {ks[i]:.3g}, c dt / m = {cs[i]:.3g}; both must be <= {STABLE} "
                             f"(an explicit spring: Mooring.for_body gives stable defaults)")

    def geometry(self, state):
        """(r, e, l, x, un) of (n, 13) states: arm, fairlead -> anchor, its length, the stretch, the approach speed."""
        s = np.asarray(state, np.float64)
        m = self.record
        r = np.einsum("nij,nj->ni", rotation_matrices(s[:, 3:7]), m[:, 3:6])
        e = m[:, 0:3] - s[:, 0:3] - r
        l = np.sqrt((e * e).sum(-1))
        u = s[:, 7:10] + np.cross(s[:, 10:13], r)
        with np.errstate(divide="ignore", invalid="ignore"):
            un = (u * e).sum(-1) / l
        return r, e, l, l - m[:, 6], un

    def tension(self, state) -> np.ndarray:
        """(n,) line tension T >= 0 (0 for a body without a line or with a slack one)."""
        m = self.record
        _, _, _, x, un = self.geometry(state)
        has = (m[:, 7] > 0.0) | (m[:, 8] > 0.0)
        with np.errstate(invalid="ignore"):
            T = np.maximum(0.0, m[:, 7] * x - m[:, 8] * un)
            return np.where(has & (x > 0.0) & (T > 0.0), T, 0.0)

    def wrench(self, state) -> np.ndarray:
        """(n, 6) line wrench [F | torque about the body origin], world frame, of (n, 13) states [p | q xyzw | v | omega], fp64."""
        r, e, l, _, _ = self.geometry(state)
        T = self.tension(state)
        with np.errstate(divide="ignore", invalid="ignore"):
            F = np.where((T > 0.0)[:, None], (T / l)[:, None] * e, 0.0)
        return np.concatenate([F, np.cross(r, F)], -1)


class MooringSpread:
    """Up to four anchored lines per body: `layers[l]` is the `Mooring` of every body's line l, `record` the (n, 9 L) array
    `ClosedLoopSim.set_mooring_spread` tiles onto the device (layer l in columns 9 l .. 9 l + 8; include/hydro.h, "Mooring
    spread").  A body with fewer lines has stiffness = damping = 0 in the layers it does not use."""

    def __init__(self, anchors, fairleads=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, n: int | None = None):
        """`anchors` (n, L, 3) world or (L, 3) for every body alike, `fairleads` likewise in the body frame (or one (3,)
        point for all lines); `length`, `stiffness`, `damping`: scalars, (L,) per line or (n, L).  `n`: from the anchors if
        they are (n, L, 3), else required.  Each layer is built as a `Mooring`, whose refusals apply per layer."""
        anchors = np.asarray(anchors, np.float64)
        if anchors.ndim not in (2, 3) or anchors.shape[-1] != 3:
            raise ValueError("mooring spread: anchors must be (L, 3) or (n, L, 3)")
        L = anchors.shape[-2]
        if not 1 <= L <= LAYERS_MAX:
            raise ValueError(f"mooring spread: a body has 1 .. {LAYERS_MAX} lines, not {L}")
        if n is None:
            if anchors.ndim != 3:
                raise ValueError("mooring spread: give n with (L, 3) anchors")
            n = anchors.shape[0]
        n = int(n)
        if n < 1:
            raise ValueError("mooring spread: n must be >= 1")
        fairleads = np.asarray(fairleads, np.float64)
        if fairleads.ndim not in (1, 2, 3) or fairleads.shape[-1] != 3:
            raise ValueError("mooring spread: fairleads must be (3,), (L, 3) or (n, L, 3)")
        try:
            a = np.broadcast_to(anchors, (n, L, 3))
            b = np.broadcast_to(fairleads, (n, L, 3))
            per_line = [np.broadcast_to(np.asarray(v, np.float64), (n, L)) for v in (length, stiffness, damping)]
        except ValueError as e:
            raise ValueError(f"mooring spread: a field does not fit {n} bodies of {L} lines ({e})") from None
        self.layers = [Mooring(a[:, l], b[:, l], length=per_line[0][:, l], stiffness=per_line[1][:, l],
                               damping=per_line[2][:, l], n=n) for l in range(L)]
        self.record = np.concatenate([m.record for m in self.layers], axis=1)

    @property
    def n(self) -> int:
        return self.record.shape[0]

    @property
    def lines(self) -> int:
        return len(self.layers)

    @property
    def anchors(self) -> np.ndarray:
        """(n, L, 3) anchors, world frame - what `ClosedLoopSim.set_mooring_spread` takes."""
        return np.stack([m.record[:, 0:3] for m in self.layers], axis=1)

    @property
    def fairleads(self) -> np.ndarray:
        """(n, L, 3) fairleads, body frame."""
        return np.stack([m.record[:, 3:6] for m in self.layers], axis=1)

    @staticmethod
    def for_body(mass, dt: float, lines: int):
        """The default (stiffness, damping) of EACH of `lines` lines on a body of `mass` stepped with `dt`: `Mooring.for_body`'s
        divided by `lines`, so that the sums over the body stand at a tenth and a half of the stability bound."""
        lines = int(lines)
        if not 1 <= lines <= LAYERS_MAX:
            raise ValueError(f"lines must be in 1 .. {LAYERS_MAX}")
        k, c = Mooring.for_body(mass, dt)
        return k / lines, c / lines

    @classmethod
    def radial(cls, lines: int, radius: float, depth: float, *, centre=(0.0, 0.0), heading: float = 0.0,
               fairlead=(0.0, 0.0, 0.0), length, stiffness, damping=0.0, n: int | None = None):
        """A symmetric spread: `lines` anchors evenly round a circle of `radius` about `centre` ((2,) or (n, 2), world x y) at
        z = -`depth`, the first at `heading` radians from +x, counter-clockwise.  One `fairlead` for all lines."""
        lines = int(lines)
        if not 1 <= lines <= LAYERS_MAX:
            raise ValueError(f"lines must be in 1 .. {LAYERS_MAX}")
        if not (np.isfinite(radius) and radius >= 0.0 and np.isfinite(depth) and np.isfinite(heading)):
            raise ValueError("mooring spread: radius must be finite and >= 0, depth and heading finite")
        centre = np.asarray(centre, np.float64)
        if centre.ndim not in (1, 2) or centre.shape[-1] != 2:
            raise ValueError("mooring spread: centre must be (2,) or (n, 2)")
        if centre.ndim == 2:
            n = centre.shape[0] if n is None else n
        if n is None:
            raise ValueError("mooring spread: give n with one centre")
        centre = np.broadcast_to(centre, (int(n), 2))
        phi = heading + 2.0 * np.pi * np.arange(lines) / lines
        anchors = np.empty((int(n), lines, 3), np.float64)
        anchors[:, :, 0] = centre[:, None, 0] + radius * np.cos(phi)[None, :]
        anchors[:, :, 1] = centre[:, None, 1] + radius * np.sin(phi)[None, :]
        anchors[:, :, 2] = -float(depth)
        return cls(anchors, fairlead, length=length, stiffness=stiffness, damping=damping, n=int(n))

    def check_stable(self, mass, dt: float) -> None:
        """ValueError if a body's lines TOGETHER break the rule of thumb: (sum k) dt^2 / m <= 0.04, (sum c) dt / m <= 0.04."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        mass = np.broadcast_to(np.asarray(mass, np.float64), (self.n,))
        tol = 1.0 + 1e-9
        ks = sum(m.record[:, 7] for m in self.layers) * dt ** 2 / mass
        cs = sum(m.record[:, 8] for m in self.layers) * dt / mass
        if (ks > STABLE * tol).any() or (cs > STABLE * tol).any():
            i = int(np.argmax(np.maximum(ks, cs)))
            raise ValueError(f"mooring spread: body {i} has (sum k) dt^2 / m = {ks[i]:.3g}, (sum c) dt / m = {cs[i]:.3g} over its "
                             f"{self.lines} lines; both must be <= {STABLE} (MooringSpread.for_body gives stable defaults)")

    def tensions(self, state) -> np.ndarray:
        """(L, n) tension of every line (0 where a line adds nothing)."""
        return np.stack([m.tension(state) for m in self.layers])

    def wrench(self, state) -> np.ndarray:
        """(n, 6) sum of the lines' wrenches on (n, 13) states, fp64."""
        return sum(m.wrench(state) for m in self.layers)
