"""The tethers of the designed population (the 321 bodies of designed_populations.bed_pop and one more), its checkers, and the
hanging pair: shared by tests/test_tether.py and tests/test_tether_gpu.py.
"""
import numpy as np

import populations
import tether_reference as tr
from designed_populations import bed_population
from mooring_population import buoy

SIZES = (200, 321, 322)
NONE_TILE, ALL_TILE = 2, 1
TIE_ULPS = (-2, -1, 1, 2)                                          # L0 - l, in ulps of l: negative = taut; once with c = 0, once with c > 0


def _layout():
    """The pairs of the population that do not depend on the states, by what they are meant to be: lists of (a, b); and the 30
    pairs of tile 1 that tether_population sorts into clamped, slack and pulling ones."""
    t1 = 64 * ALL_TILE                                             # every lane paired: 0 <-> 63, 31 <-> 32, neighbours, and mirrored lanes
    adjacent = [(t1 + a, t1 + a + 1) for a in range(1, 30, 2)]
    mirrored = [(t1 + a, t1 + 95 - a) for a in range(33, 48)]
    pull = [(t1, t1 + 63), (t1 + 31, t1 + 32)]
    slack = [(192, 199), (193, 198), (194, 197), (195, 196)]       # the live lanes of tile 3 at n = 200 pair among themselves
    for a in list(range(200, 254, 6)) + list(range(256, 316, 6)):  # 200 .. 319: in turn a pair that pulls, a slack pair, two bodies without
        pull.append((a, a + 1))
        slack.append((a + 2, a + 3))
    pull += [(316, 319), (320, 321)]                               # 320 <-> 321: the two live lanes of the last tile at n = 322
    slack += [(317, 318)]
    return pull, slack, [p for both in zip(adjacent, mirrored) for p in both]


def tether_population(st, pv, pr, seed=2028):
    """A tether per pair over 322 bodies - the 321 of tests/test_seabed_gpu.py and one more - built from each pair's own state:
    fairleads within each box, L0 = the fairleads' distance l -+ a stretch of 1e-3 .. 0.1 of min(l, 30 m), k and c per unit
    reduced mass up to 14.4 / s^2 and 1.2 / s (the defaults at 60 Hz); a pair that is to pull has its damper kept below half
    the spring's force.  Returns (state, prev, record (322, 7) float32, groups):
      tile 0 (0 .. 63)       : pairs i <-> i + 32 (every pair straddles lanes 31 | 32; every body of this tile touches the bed of
                               tests/test_seabed_gpu.py).  By what the states allow: 4 pairs within 2 fp32 ulps of L0 with c > 0
                               and the fairleads parting and 4 with c = 0 (groups 'ties_c', 'ties_0'), one pair with coincident
                               fairleads ('coincident': body i + 32 takes body i's state and fairlead, so that l2 = 0 exactly),
                               8 pairs that pull, 15 slack
      tile 1 (64 .. 127)     : every lane paired - 0 <-> 63, 31 <-> 32, neighbours, mirrored lanes; 8 taut pairs closing so fast
                               that T clamps to 0 ('clamped'), 17 pairs pull, 7 are slack
      tile 2 (128 .. 191)    : no tethers (the wave skips the evaluation)
      192 .. 199             : four slack pairs among themselves
      200 .. 319             : in turn a pair that pulls, a slack pair, two bodies without a tether
      320 <-> 321            : pulls (n = 322: the two live lanes of the last tile; record_for(rec, 321) unties body 320)."""
    n = 322
    assert len(st) == n
    rng = np.random.default_rng(seed)
    st, pv = np.array(st, np.float32), np.array(pv, np.float32)
    pr = np.asarray(pr)
    fair = rng.uniform(-0.5, 0.5, (n, 3)) * pr[:, 0:3]
    pull, slack, tile1 = _layout()
    # tile 0: classify the 32 pairs by the rate at which their fairleads part
    rec = np.zeros((n, 7))
    rec[:, 0:3] = fair
    rec[:, 6] = np.arange(n) % 64
    for a in range(32):
        rec[a, 6], rec[a + 32, 6] = a + 32, a
    for a, b in tile1:
        rec[a, 6], rec[b, 6] = b % 64, a % 64
    rate = tr.geometry(rec, st)[5]
    parting = [a for a in range(32) if rate[a] > 1e-3]
    assert len(parting) >= 4
    ties_c = parting[:4]
    rest = [a for a in range(32) if a not in ties_c]
    ties_0, coincident = rest[:4], rest[4]
    pull += [(a, a + 32) for a in rest[5:13]]
    slack += [(a, a + 32) for a in rest[13:]]
    assert len(rest[13:]) == 15
    # tile 1: the first eight pairs that close are the clamped ones, of the others seven are slack
    closing = [p for p in tile1 if rate[p[0]] < -1e-3]
    assert len(closing) >= 8
    clamped = closing[:8]
    others = [p for p in tile1 if p not in clamped]
    slack += others[:7]
    pull += others[7:]
    b = coincident + 32
    st[b], pv[b], fair[b] = st[coincident], pv[coincident], fair[coincident]
    groups = {"ties_0": [(a, a + 32) for a in ties_0], "ties_c": [(a, a + 32) for a in ties_c], "clamped": clamped,
              "coincident": [(coincident, b)], "pull": pull, "slack": slack}
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
            L0 = 0.5 if name == "coincident" else l[a] + stretch if name == "slack" else l[a] - stretch
            k = mu * rng.uniform(0.5, 14.4)
            c = mu * rng.uniform(0.0, 1.2) * (j % 5 != 0)                                 # one line in five without a damper
            rec[[a, b], 3:6] = (L0, k, c)
    rec = rec.astype(np.float32).astype(np.float64)
    _, _, _, x, _, rate = tr.geometry(rec, st64)
    for a, b in groups["pull"]:                                                           # taut and meant to pull: the damper below half the spring
        if -rec[a, 5] * rate[a] > 0.5 * rec[a, 4] * x[a]:
            rec[[a, b], 5] = 0.5 * rec[a, 4] * x[a] / -rate[a]
    for a, b in groups["clamped"]:
        rec[[a, b], 5] = 4.0 * rec[a, 4] * x[a] / -rate[a]                                # c rate = -4 k x
    for a, b in groups["ties_0"]:
        rec[[a, b], 5] = 0.0
    for a, b in groups["ties_c"]:
        rec[[a, b], 5] = max(rec[a, 5], 0.3 * m[a] * m[b] / (m[a] + m[b]))
    rec = rec.astype(np.float32)
    # the ties: L0 is the kernel's own l moved by whole fp32 steps
    free = rec.copy()
    free[:, 3] = 0.0
    l32 = tr._fp32_terms(free, st)[3]                                                     # x with L0 = 0: l itself
    for g in ("ties_0", "ties_c"):
        for (a, b), k in zip(groups[g], TIE_ULPS):
            assert l32[a] == l32[b]
            v = l32[a]
            for _ in range(abs(k)):
                v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
            rec[[a, b], 3] = v
    return st, pv, rec, {k: np.array(v) for k, v in groups.items()}


def record_for(rec, n):
    """The record of the first n bodies: a body whose partner is not among them has no tether."""
    out = np.array(rec[:n], np.float32)
    alone = tr.partner(out) >= n
    out[alone, 3:6] = 0.0
    out[alone, 6] = (np.arange(n) % 64)[alone]
    return out


def designed_population():
    """(state, prev, params f32, record, groups) of the 322 bodies, built without a device."""
    st0, pv0, pr0 = populations.integrator_population(n=4097, seed=31)
    st, pv, pr = bed_population(st0, pv0, pr0)
    st, pv, pr = (np.concatenate([a, a0[321:322]]) for a, a0 in ((st, st0), (pv, pv0), (pr, pr0)))
    st, pv, rec, groups = tether_population(st, pv, pr)
    return st, pv, pr, rec, groups


def bodies_of(groups, *names):
    return np.concatenate([groups[k].reshape(-1) for k in names])


def population_report(rec, st):
    """What the population is made of, by the fp64 reference: (taut and pulling, slack, no tether, taut and clamped)."""
    has, on, T = tr.has_tether(rec), tr.taut(rec, st), tr.tension(rec, st)
    return on & (T > 0), has & ~on, ~has, on & ~(T > 0)


def check_population(st, rec, groups):
    """The assertions on the designed population, shared with tests/test_tether_gpu.py."""
    ties = bodies_of(groups, "ties_0", "ties_c")
    for n in SIZES:
        r, s = record_for(rec, n), st[:n]
        off = ~np.isin(np.arange(n), ties)
        pulling, slack, none, clamped = population_report(r, s)
        assert (tr.taut_fp32(r, s) == tr.taut(r, s))[off].all(), n                       # the emulation agrees with the reference off the ties
        assert (pulling & off).sum() >= n / 4 and (slack & off).sum() >= n / 4 and none.sum() >= n / 4, \
            (n, (pulling & off).sum(), (slack & off).sum(), none.sum())
        assert none[64 * NONE_TILE:64 * NONE_TILE + 64].all() and tr.has_tether(r)[64 * ALL_TILE:64 * ALL_TILE + 64].all()
        j = tr.partner(r)
        assert (j < n).all() and (j[j] == np.arange(n)).all()                             # an involution among live lanes
        assert np.array_equal(r[:, 3:6], r[j, 3:6])                                       # both records of a pair carry the same constants
        lanes, mates = np.arange(n) % 64, j % 64
        tied = tr.has_tether(r)
        assert (tied & (np.abs(lanes - mates) == 1)).sum() >= 16                          # neighbours
        assert (tied & ((lanes < 32) != (mates < 32))).sum() >= 64                        # across lanes 31 | 32
        assert tied[64 * ALL_TILE] and mates[64 * ALL_TILE] == 63 and mates[64 * ALL_TILE + 31] == 32
        assert clamped[bodies_of(groups, "clamped")].all() and len(groups["clamped"]) == 8
        a, b = groups["coincident"][0]
        assert np.array_equal(s[a], s[b]) and np.array_equal(r[a, 0:3], r[b, 0:3]) and tr.has_tether(r)[a] and tr.geometry(r, s)[2][a] == 0.0
    assert not tr.has_tether(record_for(rec, 321))[320] and population_report(record_for(rec, 322), st)[0][[320, 321]].all()
    free = np.array(rec, np.float32)
    free[:, 3] = 0
    l32 = tr._fp32_terms(free, st)[3]
    for g, damped in (("ties_0", False), ("ties_c", True)):
        a = groups[g][:, 0]
        ulps = (rec[a, 3].astype(np.float64) - l32[a]) / np.spacing(l32[a])
        assert ulps.tolist() == list(TIE_ULPS) and ((rec[a, 5] > 0) == damped).all()
    assert (tr.geometry(rec, st)[5][groups["ties_c"][:, 0]] > 0).all()                    # parting: a taut tie with a damper pulls


def assert_antisymmetric(W, T, rec):
    """F_i == -F_j and T_i == T_j bit for bit for every pair of `rec`, given the probe's (n, 6) float32 W and (n,) float32 T: where
    the line pulls, each force component is the partner's with the sign bit flipped; where it does not, W and T are +0 on
    both.  Returns the number of bodies pulled."""
    W, T = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(T, np.float32)
    j = tr.partner(rec)
    pulls = T > 0
    assert np.array_equal(pulls, pulls[j]) and not (pulls & ~tr.has_tether(rec)).any()
    assert np.array_equal(T.view(np.uint32), T[j].view(np.uint32))
    F, Fj = np.ascontiguousarray(W[pulls, 0:3]), np.ascontiguousarray(W[j[pulls], 0:3])
    assert np.array_equal(F.view(np.uint32), Fj.view(np.uint32) ^ np.uint32(0x80000000))
    assert not W[~pulls].any() and not np.signbit(W[~pulls]).any() and not np.signbit(T).any()
    return int(pulls.sum())


LINE = 5.0                                                         # the hanging pair's unstretched line (m)
BOX_SIDE, BOX_MASS = 0.5, 200.0


def hanging_pair():
    """Config 1's buoy at rest at its draught and, 5 m of line below it, a heavy box (a cube of 0.5 m and 200 kg: 128.125 kg of
    water displaced) at rest: (state (2, 13), prev, params (2, 11), scene, dt, submerged weight of the box)."""
    st1, pv1, pr1, sc, dt, z_eq, mass = buoy()
    st, pv, pr = np.tile(st1, (2, 1)), np.tile(pv1, (2, 1)), np.tile(pr1, (2, 1))
    pr[1, 0:3], pr[1, 10] = BOX_SIDE, BOX_MASS
    st[1, 2] = z_eq - LINE
    weight = (BOX_MASS - sc.rho * BOX_SIDE ** 3) * sc.g
    return st, pv, pr, sc, dt, weight
