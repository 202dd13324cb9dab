"""The designed mooring spread: four layers of mooring records over the 321 bodies of tests/mooring_population.py, shared by
tests/test_mooring_spread.py and tests/test_mooring_spread_gpu.py.  A spread for n < 321 bodies is the first n rows: every line
is built from its own body's state alone.

  layer 0 : mooring_population.line_population as it stands (its eight ties, bodies 0 .. 7, are the only lines near l = L0)
  layer 1 : built from each body's own state so that a chosen stretch x gives a chosen tension T = k x (no damper), or a slack
            line, or a line whose damper clamps T to 0:
              tile 0 (0 .. 63)    : no line at all (the wave skips the layer)
              tile 1 (64 .. 127)  : a line in every lane, all pulling: 2 T0 for the even bodies, T0 / 2 for the odd ones (T0: layer
                                    0's first-step tension; a drawn line where layer 0's is clamped, 64 .. 71)
              tile 2 (128 .. 191) : layer 0 has no lines here; in turn pulling, slack, clamped, no line
              192 .. 199          : pulling (layer 0 is slack; 199 is the last live lane at n = 200)
              200 .. 319          : every other body pulling (2 T0 or T0 / 2 in turn where layer 0 pulls), the others no line
              320                 : pulling, 2 T0
  layer 2 : tile 1 from 72 on, two bodies in every eight: 4 T0 (the largest of the three) and T0 / 4 (the smallest)
  layer 3 : zeros
"""
import numpy as np

import mooring_reference as mr
import mooring_spread_reference as msr
from mooring_population import CLAMPED, designed_population, TIES

SIZES = (200, 321)
LAYERS = 4
NONE_TILE_1, ALL_TILE_1 = 0, 1                                    # layer 1: nobody has a line in tile 0, everybody in tile 1


def _line_towards(st64, b, d, L, L0, k, c):
    """(n, 9) records with fairlead b, the anchor L along the unit vectors d from the fairlead's world position."""
    rec = np.zeros((len(st64), 9))
    rec[:, 3:6] = b
    r = mr.geometry(rec, st64)[0]
    rec[:, 0:3] = st64[:, 0:3] + r + d * L[:, None]
    rec[:, 6], rec[:, 7], rec[:, 8] = L0, k, c
    return rec


def spread_population(st, pr, rec0, seed=2031):
    """(321, 36) float32: the designed spread over the states `st`, parameters `pr` and layer 0 `rec0`."""
    n = len(st)
    assert n == 321 and rec0.shape == (321, 9)
    rng = np.random.default_rng(seed)
    st64 = np.asarray(st, np.float64)
    i = np.arange(n)
    tile = i // 64
    m = pr[:, 10].astype(np.float64)
    T0 = mr.tension(rec0, st64)
    PULL, SLACK, CLAMP, NONE = 0, 1, 2, 3

    def layer(kind, target):
        """Lines of `kind` per body; `target` (n,): the tension a pulling line is to have (0: a drawn line)."""
        b = rng.uniform(-0.5, 0.5, (n, 3)) * pr[:, 0:3]
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        free = np.zeros((n, 9))
        free[:, 3:6] = b
        u = mr.geometry(free, st64)[4]
        speed = np.linalg.norm(u, axis=1)
        kind = np.where((kind == CLAMP) & (speed <= 1e-3), SLACK, kind)
        d = np.where((kind == CLAMP)[:, None], u / np.maximum(speed, 1e-30)[:, None], d)          # e along +u: the fairlead closes in
        base = rng.uniform(10.0, 30.0, n)
        x = base * 10.0 ** rng.uniform(-3.0, -1.0, n)                                            # a drawn line's stretch (or slack): 0.01 .. 3 m
        x = np.where(kind == CLAMP, 1e-3 * base, x)
        # a line with a target: k = 10 m / s^2 (inside the population's 0.5 .. 14.4) unless that makes the stretch too small to be
        # clear of the decision x > 0 - then a softer spring on 1e-3 of the length
        x = np.where(target > 0, np.maximum(target / (10.0 * m), 1e-3 * base), x)
        k = np.where(target > 0, target / x, m * rng.uniform(0.5, 14.4, n))
        L, L0 = np.where(kind == SLACK, base, base + x), np.where(kind == SLACK, base + x, base)
        rec = _line_towards(st64, b, d, L, L0, np.where(kind == NONE, 0.0, k), 0.0).astype(np.float32).astype(np.float64)
        _, _, _, xs, _, un = mr.geometry(rec, st64)
        clamp = kind == CLAMP
        rec[clamp, 8] = 4.0 * rec[clamp, 7] * xs[clamp] / un[clamp]                               # c un = 4 k x
        rec[kind == NONE] = 0.0
        return rec.astype(np.float32), kind

    kind1 = np.full(n, NONE)
    kind1[tile == 1] = PULL
    kind1[tile == 2] = (PULL, SLACK, CLAMP, NONE) * 16
    kind1[192:200] = PULL
    kind1[200:320] = np.where((i[200:320] - 200) % 2 == 0, PULL, NONE)
    kind1[320] = PULL
    factor = np.where(i % 2 == 0, 2.0, 0.5)
    factor[200:320] = np.where((i[200:320] - 200) % 4 == 0, 2.0, 0.5)
    factor[320] = 2.0
    rec1, kind1 = layer(kind1, np.where(kind1 == PULL, factor * T0, 0.0))
    kind2 = np.full(n, NONE)
    in_two = (tile == 1) & (i >= 72) & (i % 8 < 2)
    kind2[in_two] = PULL
    rec2, _ = layer(kind2, np.where(in_two, np.where(i % 8 == 0, 4.0, 0.25) * T0, 0.0))
    assert (T0[in_two] > 0).all()
    return np.concatenate([rec0.astype(np.float32), rec1, rec2, np.zeros((n, 9), np.float32)], axis=1)


def designed_spread():
    """(state, prev, params f32, spread (321, 36)) built without a device."""
    st, pv, pr, rec0 = designed_population()
    return st, pv, pr, spread_population(st, pr, rec0)


def check_spread(st, spread, n):
    """The first n bodies of the designed spread are what the tests need, by the fp64 reference.  Returns (pulls (4, n), the layer
    of each body's largest first-step tension, -1 where no line pulls)."""
    assert n in SIZES and spread.shape[1] == 9 * LAYERS and spread.dtype == np.float32
    s, sp = np.asarray(st[:n], np.float64), spread[:n]
    recs = msr.layers_of(sp)
    T = msr.tensions(sp, s)
    pulls = T > 0
    i = np.arange(n)
    tile = i // 64
    has1 = mr.has_line(recs[1])
    assert has1[tile == ALL_TILE_1].all() and pulls[1][tile == ALL_TILE_1].all()            # a line in layer 1 for every lane of a tile
    assert not has1[tile == NONE_TILE_1].any()                                              # no line in layer 1 in a whole tile
    count = pulls.sum(axis=0)
    assert (count == 2).sum() >= 16 and (count == 3).sum() >= 2 and (count == 0).sum() >= 16 and (count == 1).sum() >= 16
    slack = has1 & ~mr.taut(recs[1], s)
    clamped = mr.taut(recs[1], s) & ~pulls[1]
    assert slack.sum() >= 8 and clamped.sum() >= 4                                          # layer 1 holds slack lines and clamped lines
    assert pulls[1][n - 1]                                                                  # the last live lane of the last tile
    assert not spread[:n, 27:36].any() and not pulls[3].any()                               # layer 3: zeros
    # no body of layers 1 and 2 is near the decision x > 0: the ties stay layer 0's (bodies 0 .. 7)
    for rec in recs[1:3]:
        has = mr.has_line(rec)
        _, _, l, x, _, _ = mr.geometry(rec, s)
        assert (np.abs(x[has]) > 64 * np.spacing(l[has].astype(np.float32))).all()
    assert not has1[TIES].any() and not mr.has_line(recs[2])[TIES].any() and (TIES < 8).all() and (CLAMPED >= 64).all()
    # which layer carries the body's largest tension, unambiguously (a factor of 2 or more between the candidates)
    top = np.where(count > 0, np.argmax(T, axis=0), -1)
    ordered = np.sort(T, axis=0)
    clear = (count < 2) | (ordered[-1] > 1.5 * ordered[-2])
    assert clear.all()
    assert (top[count >= 2] == 0).sum() >= 8 and (top[count >= 2] == 1).sum() >= 8 and (top[count >= 2] == 2).sum() >= 2
    return pulls, top
