"""Tethers for the closed loop: one tension-only line between two bodies of the same tile of 64.

`Tether` builds and validates the (n, 7) record `ClosedLoopSim.set_tether` tiles onto the device and
`HydroEngine.step_fused_tiled_multi_teth` / `tether_wrench` take.  The kernels evaluate the model of include/hydro.h
("Tether") in fp32 inside every physics step, the partner's fairlead handed over between the lanes of a wavefront;
`Tether.wrench` restates it on the host in fp64 NumPy - for checking a recorded trajectory, for sizing a line.

For a body with position p, rotation R, velocity v, angular velocity omega and fairlead b (body frame), its partner with
the same primed, and a line of unstretched length L0, stiffness k and damping c:

    r    = R b,  P = p + r,  U = v + omega x r      the fairlead, world frame, and its velocity
    e    = P' - P                                   fairlead -> partner's fairlead,  l = |e|
    x    = l - L0                                   the line is taut only if x > 0
    rate = (U' - U) . e / l                         > 0: the fairleads part
    T    = max(0, k x + c rate)                     a line cannot push
    F    = T e / l,    W = (F, r x F)               and -F on the partner

A body has a tether if k > 0 or c > 0.  Both bodies of a pair lie in one tile (bodies 64 t .. 64 t + 63): the record names
the partner as a lane of that tile.  This is an explicit spring between two masses: with the reduced mass
mu = m_a m_b / (m_a + m_b), k dt^2 / mu and c dt / mu must stay at or below 0.04 (`STABLE`, the mooring's rule);
`Tether.for_pair(m_a, m_b, dt)` gives k = 0.004 mu / dt^2 and c = 0.02 mu / dt, and `check_stable` refuses a record that
breaks the rule.  Not modelled by ONE record: chains and several tethers per body - `TetherNet` below layers up to four
records, so that a string of small bodies makes a cable with mass, sag and drag.  Not modelled at all: pairs across tiles.

`TetherNet` (include/hydro.h, "Tether net") is L <= 4 layers of that record: within a layer every body has at most one line,
across the layers up to L.  The kernels of `step_fused_tiled_multi_net` evaluate the layers one after the other from the
same state and add the wrenches in ascending layer order.  A body between two springs is not a pair on its reduced mass:
the net's rule is per body, 2 (sum of k) dt^2 / m <= 0.04 and 2 (sum of c) dt / m <= 0.04 (`TetherNet.check_stable`,
`TetherNet.for_chain`).

`LinkTensions` (include/hydro.h, "Link tensions") is the view `ClosedLoopSim.track_link_tensions()` returns over the peak
tension of every line: the kernels of `step_fused_tiled_multi_peak` keep, per body and layer, the largest T a line formed in
any step - the load that sizes a cable, read off one resident run without a trajectory.
"""
from __future__ import annotations

import numpy as np

from .mooring import DEFAULT_C, DEFAULT_K, STABLE
from .seabed import rotation_matrices

FIELDS = 7                      # b(3) | L0 | k | c | partner lane
TILE = 64
LAYERS_MAX = 4                  # HYDRO_TETH_LAYERS_MAX: lines per body, layers per net


class Tether:
    def __init__(self, pairs, fairlead_a=(0.0, 0.0, 0.0), fairlead_b=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, n: int):
        """`pairs` (m, 2) body indices (a, b); `fairlead_a`, `fairlead_b` (m, 3) body frame of a and of b; `length`,
        `stiffness`, `damping` (m,) - each broadcast to the m pairs; `n`: the number of bodies of the scene.  ValueError
        for a body tied to itself, a body in two pairs, an index outside 0 .. n - 1, a pair across two tiles of 64, a
        non-finite value or a negative length, stiffness or damping."""
        n = int(n)
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            pairs = np.zeros((0, 2), np.int64)
        if pairs.ndim == 1 and pairs.shape == (2,):
            pairs = pairs[None]
        if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
            raise ValueError("tether: pairs must be (m, 2) integer body indices")
        pairs = pairs.astype(np.int64)
        m = pairs.shape[0]
        if m and (pairs.min() < 0 or pairs.max() >= n):
            raise ValueError(f"tether: a body index is outside 0 .. {n - 1}")
        for a, b in pairs:
            if a == b:
                raise ValueError(f"tether: body {a} is tied to itself")
        seen, counts = np.unique(pairs, return_counts=True)
        if (counts > 1).any():
            raise ValueError(f"tether: body {int(seen[np.argmax(counts > 1)])} is in two pairs (at most one tether per body)")
        for a, b in pairs:
            if a // TILE != b // TILE:
                raise ValueError(f"tether: bodies {a} and {b} lie in tiles {a // TILE} and {b // TILE}; a pair must lie inside one "
                                 f"block of {TILE} bodies ({TILE} t .. {TILE} t + {TILE - 1}) - lay the pair out inside one block of {TILE}")
        fa, fb = np.asarray(fairlead_a, np.float64), np.asarray(fairlead_b, np.float64)
        for f in (fa, fb):
            if f.ndim > 2 or f.shape[-1:] != (3,):
                raise ValueError("tether: a fairlead must be (3,) or (m, 3)")
        per_pair = np.empty((m, 9), np.float64)
        try:
            per_pair[:, 0:3] = fa
            per_pair[:, 3:6] = fb
            per_pair[:, 6] = np.asarray(length, np.float64)
            per_pair[:, 7] = np.asarray(stiffness, np.float64)
            per_pair[:, 8] = np.asarray(damping, np.float64)
        except ValueError as e:
            raise ValueError(f"tether: a field does not fit {m} pairs ({e})") from None
        if not np.isfinite(per_pair).all():
            raise ValueError("tether: non-finite value")
        if (per_pair[:, 6:9] < 0.0).any():
            raise ValueError("tether: length, stiffness and damping must be >= 0")
        rec = np.zeros((n, FIELDS), np.float64)
        rec[:, 6] = np.arange(n) % TILE                                     # a body without a tether names itself
        a, b = pairs[:, 0], pairs[:, 1]
        rec[a, 0:3], rec[b, 0:3] = per_pair[:, 0:3], per_pair[:, 3:6]
        rec[a, 3:6] = rec[b, 3:6] = per_pair[:, 6:9]
        rec[a, 6], rec[b, 6] = b % TILE, a % TILE
        self.pairs = pairs
        self.record = rec

    @property
    def n(self) -> int:
        return self.record.shape[0]

    @property
    def partner(self) -> np.ndarray:
        """(n,) the body each body's record names: its partner, itself without a tether."""
        i = np.arange(self.n)
        return (i // TILE) * TILE + (self.record[:, 6].astype(np.int64) & (TILE - 1))

    @staticmethod
    def for_pair(m_a, m_b, dt: float):
        """The default (stiffness, damping) of a tether between bodies of mass `m_a` and `m_b` stepped with `dt`:
        k = 0.004 mu / dt^2, c = 0.02 mu / dt with the reduced mass mu = m_a m_b / (m_a + m_b) - a tenth and a half of the
        stability bound (include/hydro.h)."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        m_a, m_b = np.asarray(m_a, np.float64), np.asarray(m_b, np.float64)
        if not (np.isfinite(m_a).all() and (m_a > 0.0).all() and np.isfinite(m_b).all() and (m_b > 0.0).all()):
            raise ValueError("mass must be finite and > 0")
        mu = m_a * m_b / (m_a + m_b)
        k, c = DEFAULT_K * mu / dt ** 2, DEFAULT_C * mu / dt
        return (float(k), float(c)) if mu.ndim == 0 else (k, c)

    def check_stable(self, mass, dt: float) -> None:
        """ValueError if a tether breaks the rule of thumb k dt^2 / mu <= 0.04, c dt / mu <= 0.04 for bodies of `mass`
        ((n,) or a scalar), mu the pair's reduced mass."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        mass = np.broadcast_to(np.asarray(mass, np.float64), (self.n,))
        if not len(self.pairs):
            return
        a, b = self.pairs[:, 0], self.pairs[:, 1]
        mu = mass[a] * mass[b] / (mass[a] + mass[b])
        tol = 1.0 + 1e-9
        ks, cs = self.record[a, 4] * dt ** 2 / mu, self.record[a, 5] * dt / mu
        if (ks > STABLE * tol).any() or (cs > STABLE * tol).any():
            i = int(np.argmax(np.maximum(ks, cs)))
            raise ValueError(f"tether: pair ({a[i]}, {b[i]}) has k dt^2 / mu = {ks[i]:.3g}, c dt / mu = {cs[i]:.3g}; both must be <= "
                             f"{STABLE} (an explicit spring on the reduced mass: Tether.for_pair gives stable defaults)")

    def geometry(self, state):
        """(r, e, l, x, rate) of (n, 13) states: arm, fairlead -> partner's fairlead, its length, the stretch, the rate at
        which the fairleads part."""
        s = np.asarray(state, np.float64)
        t, j = self.record, self.partner
        r = np.einsum("nij,nj->ni", rotation_matrices(s[:, 3:7]), t[:, 0:3])
        P = s[:, 0:3] + r
        U = s[:, 7:10] + np.cross(s[:, 10:13], r)
        e = P[j] - P
        l = np.sqrt((e * e).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            rate = ((U[j] - U) * e).sum(-1) / l
        return r, e, l, l - t[:, 3], rate

    def tension(self, state) -> np.ndarray:
        """(n,) tether tension T >= 0 (0 for a body without a tether or with a slack one); equal on both bodies of a pair."""
        t = self.record
        _, _, _, x, rate = self.geometry(state)
        has = (t[:, 4] > 0.0) | (t[:, 5] > 0.0)
        with np.errstate(invalid="ignore"):
            T = np.maximum(0.0, t[:, 4] * x + t[:, 5] * rate)
            return np.where(has & (x > 0.0) & (T > 0.0), T, 0.0)

    def wrench(self, state) -> np.ndarray:
        """(n, 6) tether wrench [F | torque about the body origin], world frame, of (n, 13) states [p | q xyzw | v | omega], fp64."""
        r, e, l, _, _ = self.geometry(state)
        T = self.tension(state)
        with np.errstate(divide="ignore", invalid="ignore"):
            F = np.where((T > 0.0)[:, None], (T / l)[:, None] * e, 0.0)
        return np.concatenate([F, np.cross(r, F)], -1)


class TetherNet:
    """Up to LAYERS_MAX tethers per body, as layers of `Tether` records: chains, cables of small bodies, bridles."""

    def __init__(self, links, fairlead_a=(0.0, 0.0, 0.0), fairlead_b=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, n: int,
                 layer=None):
        """`links` (m, 2) body indices (a, b), `fairlead_a`, `fairlead_b`, `length`, `stiffness`, `damping` as for `Tether`,
        per link.  `layer` (m,), if given, is each link's layer 0 .. 3 as it stands (two links of a layer at one body are
        refused, with Tether's message); otherwise each link, in the caller's order, gets the lowest layer that is free at
        both of its bodies.  Two links between the same two bodies are allowed (a bridle): they take two layers.
        ValueError for whatever `Tether` refuses in a layer - a body tied to itself, an index outside 0 .. n - 1, a link
        across two tiles of 64, a non-finite or negative value - and for a link that finds no free layer below 4."""
        n = int(n)
        links = np.asarray(links)
        if links.size == 0:
            links = np.zeros((0, 2), np.int64)
        if links.ndim == 1 and links.shape == (2,):
            links = links[None]
        if links.ndim != 2 or links.shape[1] != 2 or not np.issubdtype(links.dtype, np.integer):
            raise ValueError("tether: links must be (m, 2) integer body indices")
        links = links.astype(np.int64)
        m = links.shape[0]
        if m and (links.min() < 0 or links.max() >= n):
            raise ValueError(f"tether: a body index is outside 0 .. {n - 1}")
        fa, fb = np.asarray(fairlead_a, np.float64), np.asarray(fairlead_b, np.float64)
        for f in (fa, fb):
            if f.ndim > 2 or f.shape[-1:] != (3,):
                raise ValueError("tether: a fairlead must be (3,) or (m, 3)")
        per_link = np.empty((m, 9), np.float64)
        try:
            per_link[:, 0:3] = fa
            per_link[:, 3:6] = fb
            per_link[:, 6] = np.asarray(length, np.float64)
            per_link[:, 7] = np.asarray(stiffness, np.float64)
            per_link[:, 8] = np.asarray(damping, np.float64)
        except ValueError as e:
            raise ValueError(f"tether: a field does not fit {m} links ({e})") from None
        if layer is not None:
            layer = np.asarray(layer)
            if layer.shape != (m,) or not np.issubdtype(layer.dtype, np.integer):
                raise ValueError(f"tether: layer must be ({m},) integers, one per link")
            layer = layer.astype(np.int64)
            if m and (layer.min() < 0 or layer.max() >= LAYERS_MAX):
                raise ValueError(f"tether: a layer is outside 0 .. {LAYERS_MAX - 1}")
        else:
            layer = np.zeros(m, np.int64)
            taken: dict[int, set] = {}
            for i, (a, b) in enumerate(links):
                a, b = int(a), int(b)
                used = taken.setdefault(a, set()) | taken.setdefault(b, set())
                free = [l for l in range(LAYERS_MAX) if l not in used]
                if not free:
                    full = a if len(taken[a]) >= len(taken[b]) else b
                    raise ValueError(f"tether: link {i} ({a}, {b}) finds no free layer: body {full} already has "
                                     f"{len(taken[full])} lines (at most {LAYERS_MAX} lines per body, and a link needs one layer free at both ends)")
                layer[i] = free[0]
                taken[a].add(free[0])
                taken[b].add(free[0])
        self.layers = int(layer.max()) + 1 if m else 1
        self.links, self.layer = links, layer
        self.nets = []
        for l in range(self.layers):
            w = layer == l
            self.nets.append(Tether(links[w], per_link[w, 0:3], per_link[w, 3:6], length=per_link[w, 6], stiffness=per_link[w, 7],
                                    damping=per_link[w, 8], n=n))
        self.record = np.concatenate([t.record for t in self.nets], axis=1)

    @property
    def n(self) -> int:
        return self.record.shape[0]

    @classmethod
    def chain(cls, bodies, fairlead_up=(0.0, 0.0, 0.0), fairlead_down=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, n: int):
        """The chain bodies[0] - bodies[1] - ... : consecutive bodies linked, link i from `fairlead_down` of bodies[i] to
        `fairlead_up` of bodies[i + 1], in layers 0, 1, 0, 1, ... - two layers whatever the order, never three."""
        bodies = np.asarray(bodies)
        if bodies.ndim != 1 or bodies.size < 2 or not np.issubdtype(bodies.dtype, np.integer):
            raise ValueError("tether: a chain is a list of at least two body indices")
        links = np.stack([bodies[:-1], bodies[1:]], axis=1)
        return cls(links, fairlead_down, fairlead_up, length=length, stiffness=stiffness, damping=damping, n=n,
                   layer=np.arange(len(links)) % 2)

    @staticmethod
    def for_chain(masses, dt: float):
        """Uniform default (stiffness, damping) for the chain of bodies with `masses` (in the chain's order) stepped with
        `dt`: the minimum over the bodies of DEFAULT_K m_i / (2 degree_i dt^2) and of DEFAULT_C m_i / (2 degree_i dt) -
        a tenth and a half of the per-body bound of `check_stable`; degree_i is 1 at the two ends and 2 between them.
        For a lone pair this is STRICTER than `Tether.for_pair`: there the relative motion of the pair is one oscillator
        on the reduced mass mu, and k dt^2 / mu is the exact figure; here each body's row of M^-1 K is bounded on its own
        (Gershgorin: the row sum is 2 k / m_i), which for two equal masses asks k <= 0.02 m / dt^2 where the pair's rule
        allows 0.04 mu / dt^2 = 0.02 m / dt^2 - the same - and for unequal ones less, m_min / 2 against mu > m_min / 2.
        The per-body bound needs no eigenvalues and holds for every net."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        masses = np.asarray(masses, np.float64)
        if masses.ndim != 1 or masses.size < 2:
            raise ValueError("a chain has at least two bodies")
        if not (np.isfinite(masses).all() and (masses > 0.0).all()):
            raise ValueError("mass must be finite and > 0")
        degree = np.full(masses.shape, 2.0)
        degree[0] = degree[-1] = 1.0
        per_body = masses / (2.0 * degree)
        return float(DEFAULT_K * per_body.min() / dt ** 2), float(DEFAULT_C * per_body.min() / dt)

    def check_stable(self, mass, dt: float) -> None:
        """ValueError if a body breaks the net's rule of thumb, 2 (sum of k over its lines) dt^2 / m <= 0.04 and
        2 (sum of c) dt / m <= 0.04, for bodies of `mass` ((n,) or a scalar) - Gershgorin's bound on M^-1 K, body by body."""
        if not dt > 0.0:
            raise ValueError("dt must be > 0")
        mass = np.broadcast_to(np.asarray(mass, np.float64), (self.n,))
        k_sum = sum(t.record[:, 4] for t in self.nets)
        c_sum = sum(t.record[:, 5] for t in self.nets)
        ks, cs = 2.0 * k_sum * dt ** 2 / mass, 2.0 * c_sum * dt / mass
        tol = 1.0 + 1e-9
        if (ks > STABLE * tol).any() or (cs > STABLE * tol).any():
            i = int(np.argmax(np.maximum(ks, cs)))
            lines = int(sum(((t.record[i, 4] > 0.0) | (t.record[i, 5] > 0.0)) for t in self.nets))
            raise ValueError(f"tether: body {i} ({lines} lines) has 2 sum(k) dt^2 / m = {ks[i]:.3g}, 2 sum(c) dt / m = {cs[i]:.3g}; both "
                             f"must be <= {STABLE} (explicit springs, bounded body by body: TetherNet.for_chain gives stable defaults)")

    def wrench(self, state) -> np.ndarray:
        """(n, 6) the net's wrench, the fp64 sum over the layers of `Tether.wrench`."""
        return sum(t.wrench(state) for t in self.nets)

    def tensions(self, state) -> np.ndarray:
        """(m,) the tension of each link, in the caller's order."""
        out = np.zeros(len(self.links), np.float64)
        for l, t in enumerate(self.nets):
            w = self.layer == l
            out[w] = t.tension(state)[self.links[w, 0]]
        return out


class LinkTensions:
    """View over the tiled (tiles, L, 64) device record of the peak tension of every line of a `ClosedLoopSim`
    (`sim.track_link_tensions()`; include/hydro.h, "Link tensions"): row l holds, per body, the largest tension its line in
    layer l of the net has carried in any physics step since the record was last empty.  The kernels of
    `HydroEngine.step_fused_tiled_multi_peak` update it inside every step - in a resident launch the tensions between the
    first and the last step exist nowhere else.  A step's sample is the T its evaluation of the line formed where the line
    pulls (what `tether_net_wrench` returns as the tension for the state the step starts from) and +0 where it adds
    nothing; the update is the extremes record's compare-and-select: a NaN sample never enters, a NaN in the record stays,
    an equal value leaves the record's bits.  Both bodies of a link hold the same bits.  Empty is all +0.
    `buffer` is the tensor the kernels write - its address never changes; every reader waits for the step stream first.
    Not provided: when the peak occurred, minima, cycle counts."""

    def __init__(self, sim, buffer, links, layer):
        self._sim = sim
        self.buffer = buffer
        self.n = sim.n
        self.layers = int(buffer.shape[1])
        self.links = np.asarray(links, np.int64).reshape(-1, 2)
        self.layer = np.asarray(layer, np.int64).reshape(-1)

    @staticmethod
    def fold(tensions, seed=None) -> np.ndarray:
        """The host restatement: the (n, L) fp32 record after the samples `tensions` (rows, L, n) - one (L, n) set of
        per-layer tensions per step, +0 where a line adds nothing - have entered, row by row, a record that starts as
        `seed` (n, L; all +0 if None): M = T if T > M else M, bit for bit."""
        tensions = np.asarray(tensions, np.float32)
        if tensions.ndim != 3:
            raise ValueError("fold: tensions must be (rows, L, n)")
        _, layers, n = tensions.shape
        rec = np.zeros((n, layers), np.float32) if seed is None else np.array(seed, np.float32, copy=True)
        if rec.shape != (n, layers):
            raise ValueError(f"fold: seed must be ({n}, {layers})")
        with np.errstate(invalid="ignore"):
            for T in tensions:
                rec = np.where(T.T > rec, T.T, rec)
        return rec

    def record(self) -> np.ndarray:
        """(n, L) host copy of the record: the peak tension of body i's line in layer l, N (+0: it never pulled)."""
        from . import scenes
        self._sim.synchronize()
        return scenes.from_tiled(self.buffer.cpu().numpy(), self.n)

    def peak(self, record=None) -> np.ndarray:
        """(m,) the peak tension of each link, in the caller's order of `set_tether_net` / `set_tether`: read at the link's
        first body, links[:, 0], in the link's layer (`TetherNet.tensions`' convention; the other end holds the same bits)."""
        rec = self.record() if record is None else np.asarray(record)
        return rec[self.links[:, 0], self.layer]

    def reset(self) -> None:
        """Start over from the empty record (all +0), on the sim's stream."""
        import torch
        with torch.cuda.stream(self._sim.stream):
            self.buffer.zero_()
