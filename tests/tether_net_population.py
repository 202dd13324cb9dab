"""The tether net of the designed population, its checker, and the hanging chain: shared by tests/test_tether_net.py and
tests/test_tether_net_gpu.py.  It wraps tests/tether_population.py, which stays as it is.

THE NET is four layers over the 322 bodies of tether_population.designed_population (n = 200, 321, 322 as there):
  layer 0 : section 22's record, exactly as tether_population builds it (the ties, the clamped and the coincident pair included)
  layer 1 : built from the bodies' own states like layer 0 (fairleads within each box, L0 = the fairleads' distance -+ a stretch
            of 1e-3 .. 0.1 of min(l, 30 m), k and c per unit reduced mass up to 14.4 / s^2 and 1.2 / s):
              tile 0   : the eight pairs (a, a + 32) that PULL in layer 0 are closed into a ring by eight links that pull,
                         (a + 32 of one pair, a of the next): sixteen bodies, alternately a line of layer 0 and a line of layer 1,
                         every one of them across lanes 31 | 32 - any eight consecutive bodies of it are a chain; and two slack
                         links between bodies of layer 0's slack pairs
              tile 1   : NO line (every lane has one in layer 0: the wave skips layer 1 only)
              tile 2   : every lane paired - 0 <-> 63, 31 <-> 32 and neighbours - where layer 0 has no line (the wave skips layer 0
                         only): the first four pairs that close fast are CLAMPED, eight are slack, the others pull
              tile 3   : (n >= 321) the open chain 218 - 219 - 220 - 221 - 224 - 225 - 226 - 227, layer 0's (218, 219), (220, 221),
                         (224, 225), (226, 227) joined by layer 1's (219, 220), (221, 224) - across lanes 31 | 32 - and (225, 226);
                         and links from one pulling pair of layer 0 to the next
              tile 4   : links from one pulling pair of layer 0 to the next; tile 5: no line
  layer 2 : ONE pair that pulls, (8, 11) - body 8 has three lines
  layer 3 : all zeros (a body names itself)
Nothing in layers 1 .. 3 is within 1e-3 of its L0: what a test may leave out stays the sixteen bodies at layer 0's ties.

BODIES PULLED IN BOTH LAYERS 0 AND 1.  The layout asks for n / 8 of them.  With layer 0 as it stands and no line of layer 1 in
tile 1 that is possible at n = 321 and 322 only: at n = 200 layer 0 pulls 24 bodies outside tile 1 (tile 0's eight pulling pairs
and the taut half of its eight ties), fewer than 200 / 8 = 25.  The checker asks n / 8 at 321 and 322 and, at n = 200, ALL sixteen
bodies of tile 0's pulling pairs (the ring).
"""
import numpy as np

import tether_reference as tr
import tether_net_reference as tnr
from mooring_population import buoy
from tether_population import bodies_of, designed_population, record_for, SIZES  # noqa: F401  (SIZES is re-exported)

LAYERS = 4
NO_LAYER1_TILE, ONLY_LAYER1_TILE = 1, 2
OPEN_CHAIN = (218, 219, 220, 221, 224, 225, 226, 227)
LAYER2_PAIR = (8, 11)


def _layer(st, pr, groups, rng, fair):
    """An (n, 7) float32 record with the links of `groups` ('pull', 'slack', 'clamped': lists of (a, b)), built from the states
    as tether_population builds layer 0."""
    n = len(st)
    rec = np.zeros((n, 7))
    rec[:, 0:3] = fair
    rec[:, 6] = np.arange(n) % 64
    pairs = np.array([p for g in groups.values() for p in g])
    assert len(np.unique(pairs)) == pairs.size and (pairs[:, 0] // 64 == pairs[:, 1] // 64).all()
    rec[pairs[:, 0], 6], rec[pairs[:, 1], 6] = pairs[:, 1] % 64, pairs[:, 0] % 64
    st64 = st.astype(np.float64)
    l = tr.geometry(rec, st64)[2]
    m = pr[:, 10].astype(np.float64)
    for name, g in groups.items():
        for j, (a, b) in enumerate(g):
            mu = m[a] * m[b] / (m[a] + m[b])
            stretch = (1e-3 if name == "clamped" else 10.0 ** rng.uniform(-3.0, -1.0)) * min(l[a], 30.0)
            L0 = l[a] + stretch if name == "slack" else l[a] - stretch
            rec[[a, b], 3:6] = (L0, mu * rng.uniform(0.5, 14.4), mu * rng.uniform(0.0, 1.2) * (j % 5 != 0))
    rec = rec.astype(np.float32).astype(np.float64)
    _, _, _, x, _, rate = tr.geometry(rec, st64)
    for a, b in groups.get("pull", []):                               # meant to pull: the damper below half the spring
        if -rec[a, 5] * rate[a] > 0.5 * rec[a, 4] * x[a]:
            rec[[a, b], 5] = 0.5 * rec[a, 4] * x[a] / -rate[a]
    for a, b in groups.get("clamped", []):
        rec[[a, b], 5] = 4.0 * rec[a, 4] * x[a] / -rate[a]            # c rate = -4 k x
    return rec.astype(np.float32)


def net_population(seed=2030):
    """(state, prev, params f32, net (322, 28) float32, groups): tether_population.designed_population with the net of the module's
    docstring; groups: layer 0's, and 'pull1', 'slack1', 'clamped1', 'ring' (the sixteen bodies, in the ring's order)."""
    st, pv, pr, rec0, groups = designed_population()
    n = len(st)
    rng = np.random.default_rng(seed)
    fair = rng.uniform(-0.5, 0.5, (n, 3)) * pr[:, 0:3]
    # tile 0: the ring through layer 0's pulling pairs
    heads = [int(a) for a, b in groups["pull"] if a < 64]
    assert len(heads) == 8 and all(int(b) == a + 32 for a, b in groups["pull"] if a < 64)
    pull = [(heads[i] + 32, heads[(i + 1) % 8]) for i in range(8)]
    ring = [b for a in heads for b in (a, a + 32)]
    idle0 = [int(a) for a, b in groups["slack"] if a < 64]
    slack = [(idle0[0], idle0[1] + 32), (idle0[2], idle0[3] + 32)]
    # tile 2: every lane paired; classified by the rate at which the fairleads part
    t2 = 64 * ONLY_LAYER1_TILE
    tile2 = [(t2, t2 + 63), (t2 + 31, t2 + 32)] + [(t2 + a, t2 + a + 1) for a in range(1, 30, 2)] + [(t2 + a, t2 + a + 1) for a in range(33, 62, 2)]
    probe = np.zeros((n, 7))
    probe[:, 0:3] = fair
    probe[:, 6] = np.arange(n) % 64
    for a, b in tile2:
        probe[a, 6], probe[b, 6] = b % 64, a % 64
    rate = tr.geometry(probe, st)[5]
    closing = [p for p in tile2 if rate[p[0]] < -1e-3]
    assert len(closing) >= 4
    clamped = closing[:4]
    others = [p for p in tile2 if p not in clamped]
    slack += others[:8]
    pull += others[8:]
    # tiles 3 and 4: the open chain, and links from one pulling pair of layer 0 to the next
    pull += [(219, 220), (221, 224), (225, 226)]
    pull += [(201, 206), (207, 212), (213, 218), (231, 236), (237, 242), (243, 248)]
    pull += [(a + 1, a + 6) for a in range(256, 305, 6)]
    slack += [(311, 316)]
    rec1 = _layer(st, pr, {"pull": pull, "slack": slack, "clamped": clamped}, rng, fair)
    rec2 = _layer(st, pr, {"pull": [LAYER2_PAIR]}, rng, rng.uniform(-0.5, 0.5, (n, 3)) * pr[:, 0:3])
    rec2[~tr.has_tether(rec2), 0:3] = 0.0
    rec3 = np.zeros((n, 7), np.float32)
    rec3[:, 6] = np.arange(n) % 64
    net = np.concatenate([rec0, rec1, rec2, rec3], axis=1)
    groups = dict(groups, pull1=np.array(pull), slack1=np.array(slack), clamped1=np.array(clamped), ring=np.array(ring))
    return st, pv, pr, net, groups


def net_for(net, n, layers=None):
    """The net of the first n bodies, `layers` of its layers (default: all): tether_population.record_for, layer by layer."""
    recs = tnr.layers_of(net)[:layers]
    return np.concatenate([record_for(r, n) for r in recs], axis=1)


def check_net(st, net, groups):
    """The assertions on the designed net, by the fp64 reference, for each n."""
    ties = bodies_of(groups, "ties_0", "ties_c")
    assert len(ties) == 16 and net.shape == (322, 7 * LAYERS) and net.dtype == np.float32
    assert np.array_equal(net[:, 0:7], designed_population()[3])                          # layer 0 is section 22's record
    for n in SIZES:
        full, s = net_for(net, n), st[:n]
        recs = tnr.layers_of(full)
        lanes = np.arange(n) % 64
        for l, r in enumerate(recs):                                                      # every layer is a valid record of section 22
            j = tr.partner(r)
            assert (j < n).all() and (j[j] == np.arange(n)).all() and np.array_equal(r[:, 3:6], r[j, 3:6]), (n, l)
            if l:                                                                         # and nothing but layer 0's sixteen is near a tie
                assert np.array_equal(tr.taut_fp32(r, s), tr.taut(r, s)), (n, l)
                x, length = tr.geometry(r, s)[3], tr.geometry(r, s)[2]
                assert (np.abs(x[tr.has_tether(r)]) >= 0.9e-3 * np.minimum(length[tr.has_tether(r)], 30.0)).all(), (n, l)
        has = np.stack([tr.has_tether(r) for r in recs])
        pulls, T = tnr.pulls(full, s), tnr.tensions(full, s)
        tile = lambda t: slice(64 * t, 64 * t + 64)  # noqa: E731
        # layer 1: pairs in the tile layer 0 leaves empty, none in the tile layer 0 fills
        assert has[1][tile(ONLY_LAYER1_TILE)].all() and not has[0][tile(ONLY_LAYER1_TILE)].any()
        assert not has[1][tile(NO_LAYER1_TILE)].any() and has[0][tile(NO_LAYER1_TILE)].all()
        mates1 = tr.partner(recs[1]) % 64
        t2 = 64 * ONLY_LAYER1_TILE
        assert mates1[t2] == 63 and mates1[t2 + 31] == 32
        # slack and clamped lines in layer 1
        on1 = tr.taut(recs[1], s)
        assert (has[1] & ~on1).sum() >= 16 and (on1 & ~pulls[1]).sum() == 8 and on1[bodies_of(groups, "clamped1")].all()
        assert not pulls[1][bodies_of(groups, "clamped1")].any()
        # the ring of tile 0: sixteen bodies, alternately a line of layer 0 and of layer 1, every link across lanes 31 | 32 and pulling
        ring = groups["ring"]
        j0, j1 = tr.partner(recs[0]), tr.partner(recs[1])
        for i in range(16):
            a, b = ring[i], ring[(i + 1) % 16]
            assert (j0[a] == b) if i % 2 == 0 else (j1[a] == b), (n, i)
            assert (lanes[a] < 32) != (lanes[b] < 32)
        assert pulls[0][ring].all() and pulls[1][ring].all() and not np.isin(ring, ties).any()
        if n >= 321:                                                                      # the open chain of tile 3 across lanes 31 | 32
            for i, (a, b) in enumerate(zip(OPEN_CHAIN[:-1], OPEN_CHAIN[1:])):
                assert (j0[a] == b) if i % 2 == 0 else (j1[a] == b and pulls[1][a]), (n, i)
            assert lanes[221] == 29 and lanes[224] == 32
        # bodies pulled in both layers: n / 8 where layer 0 allows it (the module's docstring), the whole ring at n = 200
        both = pulls[0] & pulls[1]
        outside = np.ones(n, bool)
        outside[tile(NO_LAYER1_TILE)] = False
        if n == 200:
            assert (pulls[0] & outside).sum() == 24 < n / 8 and (both & ~np.isin(np.arange(n), ties)).sum() == 16, (n, both.sum())
        else:
            assert both.sum() >= n / 8, (n, both.sum())
        # layer 2: one pair, and it pulls; layer 3: zeros
        assert has[2].sum() == 2 and pulls[2][list(LAYER2_PAIR)].all() and tr.partner(recs[2])[LAYER2_PAIR[0]] == LAYER2_PAIR[1]
        assert not recs[3][:, 0:6].any() and np.array_equal(recs[3][:, 6], lanes.astype(np.float32))
        assert (has.sum(axis=0) == 3).sum() >= 1 and T[2][LAYER2_PAIR[0]] == T[2][LAYER2_PAIR[1]]


# ---- the hanging chain ------------------------------------------------------------------------------------------------------------
LINK = 1.25                                                        # each link's unstretched length (m)
BOX_SIDE, BOX_MASS, BOXES = 0.25, 25.0, 4
# The fp64 run of this scene through tether_net_reference.closed_loop_net (implicit drag, k and c at half the per-body stability
# bound) shows after 3600 steps |T - weight| <= 0.0362 N and |v| <= 2.02e-4 m/s (tests/test_tether_net.py prints them): the
# thresholds, on the host and on the device, are twice those figures.
HANG_STEPS, HANG_SPEED, HANG_TENSION = 3600, 4.04e-4, 0.0724


def hanging_chain():
    """Config 1's buoy at rest at its draught and, below it, four boxes (cubes of 0.25 m and 25 kg: 16.015625 kg of water
    displaced each) at rest, 1.25 m apart: (state (5, 13), prev, params (5, 11), scene, dt, the submerged weight hanging below each
    of the four links - 4, 3, 2 and 1 boxes)."""
    st1, pv1, pr1, sc, dt, z_eq, mass = buoy()
    k = BOXES + 1
    st, pv, pr = np.tile(st1, (k, 1)), np.tile(pv1, (k, 1)), np.tile(pr1, (k, 1))
    pr[1:, 0:3], pr[1:, 10] = BOX_SIDE, BOX_MASS
    st[1:, 2] = z_eq - LINK * np.arange(1, k)
    weight = (BOX_MASS - sc.rho * BOX_SIDE ** 3) * sc.g
    return st, pv, pr, sc, dt, weight * np.arange(BOXES, 0, -1)


def hanging_constants(pr, dt):
    """(k, c) of the hanging chain: uniform, at HALF the per-body stability bound 2 sum(k) dt^2 / m, 2 sum(c) dt / m <= 0.04 of its
    lightest interior body (two lines on 25 kg): k = 450 N/m, c = 7.5 N s/m at dt = 1/60."""
    m, stable = float(pr[1:, 10].min()), 0.04
    return 0.5 * stable * m / (4.0 * dt ** 2), 0.5 * stable * m / (4.0 * dt)
