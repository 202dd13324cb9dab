"""Per-body response statistics of a closed-loop run: mean, standard deviation and up-crossing rate of two channels.

A peak (`extremes`) is the largest sample of one random realisation of an irregular sea; a mooring designer also takes the
mean and the standard deviation of the response and its mean up-crossing rate: from them come the mean offset and the mean
tension, the significant response 2 sigma, the zero-up-crossing period Tz = duration / up-crossings, the most probable
maximum mu + sigma * sqrt(2 ln N_up) of a storm of any length (Rayleigh), and - on the tension channel against the level 0 -
the number of slack-to-taut events of a line.  The kernels of `HydroEngine.step_fused_tiled_multi_stat` keep the sums, per
body and for two channels, and update them after EVERY physics step inside the launch (include/hydro.h, "Statistics").

Channels: x, y, z (s[0..2]), vx, vy, vz (s[7..9]) and tension - exactly the tension the extremes record samples: the T the
body's mooring line or spread formed in that step, +0 where no line pulls.  Each slot (a, b) has a reference level L per body.

The record, per tile of 64 bodies: `{ double sums[4][64]; uint32 words[3][64]; }` = 2 816 B, 44 B per body:
    sums  = S1_a, S2_a, S1_b, S2_b     the sums of d and d * d, d = sample - level
    words = up_a, up_b, n              the two up-crossing words and the number of samples

The arithmetic, per slot and step, x the fp32 sample and L the fp32 level - plain IEEE double, one rounding per operation,
no fused multiply-add, so `fold` reproduces the device's bits with NumPy float64:
    d = float64(x) - float64(L);   S1 = S1 + d;   q = d * d;   S2 = S2 + q
    above = x > L  (fp32, false for a NaN).  Bit 31 of an up-crossing word: "the last sample was not above its level";
    bits 0..30: the count.  If bit 31 is set and `above`, count += 1; then bit 31 = not above.  A reset record has bit 31
    clear: the first sample never counts; x == L is not above.
n grows by the launch's `steps` at the end of every launch.  A NaN sample poisons that body's sums of that slot only.

Not provided: heave relative to the moving surface, covariances between channels, more than two channels per record,
statistics of the wrench, per-link statistics of tether nets.  The record does not remember its channels or levels.
"""
from __future__ import annotations

import numpy as np

CHANNELS = ("x", "y", "z", "vx", "vy", "vz", "tension")
X, Y, Z, VX, VY, VZ, TENSION = range(7)
INDEX = dict(zip(CHANNELS, range(7)))
STATE_FIELD = (0, 1, 2, 7, 8, 9)                 # the state field a motion or velocity channel samples
BYTES_PER_BODY = 44
FIELDS = BYTES_PER_BODY // 4                     # the tiled record in 4-byte fields: (tiles, 11, 64)
TILE = 64
LAST_BELOW = np.uint32(0x80000000)               # bit 31 of an up-crossing word
COUNT_MASK = np.uint32(0x7FFFFFFF)


def channel_index(ch) -> int:
    """A channel as its number: a name of `CHANNELS` or 0 .. 6."""
    if isinstance(ch, str):
        if ch not in INDEX:
            raise ValueError(f"unknown statistics channel {ch!r} (one of {CHANNELS})")
        return INDEX[ch]
    ch = int(ch)
    if not 0 <= ch < len(CHANNELS):
        raise ValueError(f"statistics channel {ch} out of range 0 .. {len(CHANNELS) - 1}")
    return ch


def samples_of(states, tensions, ch) -> np.ndarray:
    """(rows, n) fp32 samples of channel `ch` from recorder rows `states` (rows, n, 13) and per-step `tensions` (rows, n)."""
    ch = channel_index(ch)
    if ch == TENSION:
        return np.asarray(tensions, np.float32)
    return np.asarray(states, np.float32)[:, :, STATE_FIELD[ch]]


def empty(n: int) -> dict:
    """The reset record of n bodies as host arrays: `sums` (n, 4) float64 of +0.0, `up` (n, 2) uint32 of 0, `n` (n,) uint32 of 0."""
    n = int(n)
    return {"sums": np.zeros((n, 4), np.float64), "up": np.zeros((n, 2), np.uint32), "n": np.zeros(n, np.uint32)}


def unpack(tiled, n: int) -> dict:
    """The (tiles, 11, 64) float32 device record (as a host array) as the dict of `empty`: the tile's bytes are
    `double sums[4][64]` then `uint32 words[3][64]`."""
    raw = np.ascontiguousarray(np.asarray(tiled, np.float32))
    tiles = raw.shape[0]
    if raw.shape[1:] != (FIELDS, TILE) or tiles * TILE < n:
        raise ValueError(f"expected a (>= {(n + TILE - 1) // TILE}, {FIELDS}, {TILE}) float32 record")
    b = raw.view(np.uint8).reshape(tiles, FIELDS * TILE * 4)
    sums = np.ascontiguousarray(b[:, :4 * TILE * 8]).view(np.float64).reshape(tiles, 4, TILE)
    words = np.ascontiguousarray(b[:, 4 * TILE * 8:]).view(np.uint32).reshape(tiles, 3, TILE)
    sums = sums.transpose(0, 2, 1).reshape(tiles * TILE, 4)[:n]
    words = words.transpose(0, 2, 1).reshape(tiles * TILE, 3)[:n]
    return {"sums": sums.copy(), "up": words[:, :2].copy(), "n": words[:, 2].copy()}


def pack(record, tiles: int | None = None) -> np.ndarray:
    """`unpack`'s inverse: the dict as a (tiles, 11, 64) float32 array (padding lanes zero)."""
    sums, up, cnt = (np.asarray(record["sums"], np.float64), np.asarray(record["up"], np.uint32), np.asarray(record["n"], np.uint32))
    n = sums.shape[0]
    tiles = (n + TILE - 1) // TILE if tiles is None else int(tiles)
    s = np.zeros((tiles * TILE, 4), np.float64)
    w = np.zeros((tiles * TILE, 3), np.uint32)
    s[:n] = sums
    w[:n, :2] = up
    w[:n, 2] = cnt
    out = np.zeros((tiles, FIELDS * TILE * 4), np.uint8)
    out[:, :4 * TILE * 8] = np.ascontiguousarray(s.reshape(tiles, TILE, 4).transpose(0, 2, 1)).view(np.uint8).reshape(tiles, -1)
    out[:, 4 * TILE * 8:] = np.ascontiguousarray(w.reshape(tiles, TILE, 3).transpose(0, 2, 1)).view(np.uint8).reshape(tiles, -1)
    return out.view(np.float32).reshape(tiles, FIELDS, TILE)


def fold(record, samples_a, samples_b, levels) -> dict:
    """The header's arithmetic in NumPy: the record after the fp32 samples `samples_a`, `samples_b` (rows, n) have entered,
    row by row, a record that starts as `record` (the dict of `empty`; None: the reset record) against `levels` (n, 2) fp32.
    `n` grows by the number of rows.  Bit for bit what the kernel leaves after launches of `rows` steps in all."""
    a = np.asarray(samples_a, np.float32)
    b = np.asarray(samples_b, np.float32)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("fold: samples_a and samples_b must both be (rows, n)")
    n = a.shape[1]
    lev = np.asarray(levels, np.float32)
    if lev.shape != (n, 2):
        raise ValueError(f"fold: levels must be ({n}, 2)")
    rec = empty(n) if record is None else {k: np.array(v, copy=True) for k, v in record.items()}
    sums, up = rec["sums"].astype(np.float64, copy=False), rec["up"].astype(np.uint32, copy=False)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, xs in enumerate((a, b)):
            L32 = lev[:, c]
            L = L32.astype(np.float64)
            for x in xs:
                d = x.astype(np.float64) - L
                sums[:, 2 * c] = sums[:, 2 * c] + d
                q = d * d
                sums[:, 2 * c + 1] = sums[:, 2 * c + 1] + q
                above = x > L32
                w = up[:, c]
                count = (w + ((w >> np.uint32(31)) & above.astype(np.uint32))) & COUNT_MASK
                up[:, c] = count | np.where(above, np.uint32(0), LAST_BELOW)
    rec["sums"], rec["up"] = sums, up
    rec["n"] = (rec["n"].astype(np.uint64) + np.uint64(a.shape[0])).astype(np.uint32)
    return rec


def mean(record, slot: int, levels) -> np.ndarray:
    """(n,) mean of slot 0 / 1: L + S1 / n (NaN before the first sample)."""
    cnt = np.asarray(record["n"], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(levels, np.float32)[:, slot].astype(np.float64) + record["sums"][:, 2 * slot] / cnt


def variance(record, slot: int) -> np.ndarray:
    """(n,) population variance of slot 0 / 1: S2 / n - (S1 / n)^2, not below 0.  The sums are taken about the level, so
    with a level near the mean nothing cancels."""
    cnt = np.asarray(record["n"], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = record["sums"][:, 2 * slot] / cnt
        v = record["sums"][:, 2 * slot + 1] / cnt - m * m
    return np.where(v < 0.0, 0.0, v)


def upcrossings(record, slot: int) -> np.ndarray:
    """(n,) up-crossings of slot 0 / 1 counted so far: bits 0 .. 30 of its word."""
    return (np.asarray(record["up"], np.uint32)[:, slot] & COUNT_MASK).astype(np.int64)


class ResponseStatistics:
    """View over the two device buffers of a `ClosedLoopSim` (`sim.track_statistics()`): `buffer` is the statistics record
    the kernels read and write, `levels_buffer` the tiled (tiles, 2, 64) levels they read - the addresses never change; every
    reader waits for the step stream first.  `channels` are the two channel names, `levels` the (n, 2) host levels."""

    fold = staticmethod(fold)
    empty = staticmethod(empty)

    def __init__(self, sim, buffer, levels_buffer, channels, levels):
        self._sim = sim
        self.buffer = buffer
        self.levels_buffer = levels_buffer
        self.n = sim.n
        self.channels = tuple(CHANNELS[channel_index(c)] for c in channels)
        self.levels = np.array(levels, np.float32, copy=True)

    @staticmethod
    def channel_names(numbers):
        return tuple(CHANNELS[channel_index(c)] for c in numbers)

    @property
    def channel_numbers(self):
        return tuple(INDEX[c] for c in self.channels)

    def _slot(self, ch) -> int:
        name = CHANNELS[channel_index(ch)]
        if name not in self.channels:
            raise ValueError(f"channel {name!r} is not tracked (tracked: {self.channels})")
        return self.channels.index(name)

    def record(self) -> dict:
        """Host copy of the record: the dict of `empty` (`sums` (n, 4), `up` (n, 2), `n` (n,))."""
        self._sim.synchronize()
        return unpack(self.buffer.cpu().numpy(), self.n)

    def count(self) -> np.ndarray:
        """(n,) samples taken so far."""
        return self.record()["n"].astype(np.int64)

    def mean(self, ch) -> np.ndarray:
        return mean(self.record(), self._slot(ch), self.levels)

    def variance(self, ch) -> np.ndarray:
        return variance(self.record(), self._slot(ch))

    def std(self, ch) -> np.ndarray:
        return np.sqrt(self.variance(ch))

    def upcrossings(self, ch) -> np.ndarray:
        return upcrossings(self.record(), self._slot(ch))

    def tz(self, ch, dt: float) -> np.ndarray:
        """(n,) zero-up-crossing period about the level, s: duration / up-crossings (inf where there were none)."""
        rec = self.record()
        up = upcrossings(rec, self._slot(ch)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return rec["n"].astype(np.float64) * float(dt) / up

    def most_probable_maximum(self, ch, steps=None) -> np.ndarray:
        """(n,) mean + std * sqrt(2 ln N_up), the most probable maximum of a narrow-banded Gaussian response (Rayleigh peaks)
        over the recorded duration - or, with `steps`, over a duration of that many steps at the recorded up-crossing rate.
        The mean where N_up <= 1."""
        rec = self.record()
        slot = self._slot(ch)
        n_up = upcrossings(rec, slot).astype(np.float64)
        if steps is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                n_up = n_up * float(steps) / rec["n"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            factor = np.sqrt(2.0 * np.log(np.where(n_up > 1.0, n_up, 1.0)))
        return mean(rec, slot, self.levels) + np.sqrt(variance(rec, slot)) * factor

    def reset(self) -> None:
        """Start over, on the sim's stream: sums +0.0, words 0.  The levels and channels stay."""
        import torch
        sim = self._sim
        with torch.cuda.stream(sim.stream):
            sim.engine.statistics_reset(self.buffer, sim.n)
        sim._statistics_dirty = False
