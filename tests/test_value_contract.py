"""The tables and checkers of tests/value_contract.py, shown on the host: the tables are what they claim, the checkers pass on the
fp32 restatements of include/hydro.h standing in for the device, and each of five mutations of those restatements fails at least
one assertion:
    np.fmin / np.fmax in place of the compare-and-select           -> check_extremes
    "has a line" as not (k <= 0)                                   -> check_probe (a), on the damper-only row
    a dead partner that answers a non-zero value                   -> check_probe (c)
    +0 added to a wrench that is to be left untouched              -> assert_same_bits on the wrench a step logs
    the partner taken modulo 64 after rounding to nearest          -> check_probe (c), on partner + 0.7
The conditions on the malformed-record table are asserted here and are not measured on the device: every finite case decides
x > 0 with a margin of 2^-10 (l + |L0|), and the fp64 reference and the fp32 emulation decide alike on EVERY case lane.
The pose-hold restatement follows the header's comparison `n2 > f_max * f_max` literally: false for a NaN.
"""
import numpy as np
import pytest

import mooring_population as mp
import mooring_reference as mr
import pose_hold_reference as phr
import tether_net_population as tnp
import tether_population as tp
import tether_reference as tr
import value_contract as vc
from silver2_isaacsim_amd.extremes import Extremes


@pytest.fixture(scope="module")
def tethers():
    st, pv, pr, rec, groups = tp.designed_population()
    return st, pv, rec, groups, {n: vc.malformed_tethers(rec, st, groups["pull"], n) for n in vc.SIZES}


@pytest.fixture(scope="module")
def lines():
    st, pv, pr = (a[:321] for a in tnp.net_population()[:3])        # (the bodies the device tests moor: the net's, whose coincident pair shares a state)
    rec = mp.line_population(st, pr)
    pulling = np.flatnonzero(mp.population_report(rec, st)[0] & mp.OFF_TIES)
    return st, pv, rec, {n: vc.malformed_lines(rec, st, pulling, n) for n in vc.SIZES}


# ---- 1. the poison table -----------------------------------------------------------------------------------------------------------------
def test_the_poison_table_is_what_it_claims():
    st, pv, _, _ = mp.designed_population()
    assert np.isfinite(st).all() and np.isfinite(pv).all()
    for n in vc.SIZES:
        ps, pp, bodies, names = vc.poison(st, pv, n)
        assert 10 <= len(bodies) <= 12 and len(set(bodies.tolist())) == len(bodies) and set(names) == {p[0] for p in vc.POISONS}
        full = bodies[bodies < 64 * (n // 64)]
        assert {0, 31, 32, 63} <= set((full % 64).tolist()) and {64 * ((n - 1) // 64), n - 1} <= set(bodies.tolist())
        others = ~np.isin(np.arange(n), bodies)
        assert vc.same_bits(ps[others], st[:n][others]) and vc.same_bits(pp[others], pv[:n][others])
        for b, name in zip(bodies, names):                         # ONE poison per body, in the columns the table names
            _, where, cols, value = next(p for p in vc.POISONS if p[0] == name)
            got, was = (ps, st) if where == "state" else (pp, pv)
            changed = np.flatnonzero(vc.bits(got[b]) != vc.bits(was[b]))
            assert set(changed.tolist()) <= set(cols) and len(changed) >= 1, (b, name)
            assert vc.same_bits(got[b, list(cols)], np.full(len(cols), value, np.float32))
            other = pp if where == "state" else ps
            assert vc.same_bits(other[b], (pv if where == "state" else st)[b])
        big = ps[bodies[names.index("huge_velocity")], 8]
        with np.errstate(over="ignore"):
            assert np.isfinite(big) and np.isinf(big * big)
    assert np.isnan(vc.PAYLOAD_NAN) and vc.bits(vc.PAYLOAD_NAN)[0] == 0x7fc01234 and np.isnan(vc.NEGATIVE_NAN) and np.signbit(vc.NEGATIVE_NAN)


def test_the_poisoned_bodies_are_untied_in_every_layer():
    st, pv, pr, net, groups = tnp.net_population()
    for n in vc.SIZES:
        bodies = vc.poisoned_bodies(n)
        full = tnp.net_for(net, n)
        loose = vc.untie(full, bodies)
        vc.assert_untied(loose, bodies)
        with pytest.raises(AssertionError):
            vc.assert_untied(full, bodies)
        for l, rec in enumerate(np.split(loose, 4, axis=1)):       # still a valid record, and most lines are still there
            j = tr.partner(rec)
            assert (j < n).all() and (j[j] == np.arange(n)).all()
        assert tr.has_tether(loose[:, 0:7]).sum() >= tr.has_tether(full[:, 0:7]).sum() - 2 * len(bodies)


def test_assert_isolated_sees_one_bit_in_one_clean_body():
    st = mp.designed_population()[0][:200]
    bodies = vc.poisoned_bodies(200)
    got = st.copy()
    got[bodies] = np.nan
    assert vc.assert_isolated(got, st, bodies) == 200 - len(bodies)
    got[5, 3] = np.nextafter(got[5, 3], np.float32(2))
    with pytest.raises(AssertionError):
        vc.assert_isolated(got, st, bodies)
    zero = np.zeros((4, 2), np.float32)
    with pytest.raises(AssertionError):                            # -0 is not +0
        vc.assert_same_bits(-zero, zero)


def test_the_pose_hold_restatement_compares_as_the_header_does():
    """if (n2 > f_max * f_max): false for a NaN f_max (no clamp), true for 0 whenever the force is not (a zero comes out), and for a
    negative f_max where n2 > f_max^2 - the force comes out turned round, with the norm |f_max|."""
    rng = np.random.default_rng(5)
    n = 64
    st = rng.normal(size=(n, 13)).astype(np.float32)
    ctl = phr.record(n, rng.normal(size=(n, 3)), rng.normal(size=(n, 4)), rng.uniform(1, 5, (n, 3)), rng.uniform(0, 1, (n, 3)), 2.0, 0.5)
    free = phr.unclamped(st, ctl)[0]
    norm = np.linalg.norm(free, axis=1)
    for value, want, acts in ((np.nan, free, False), (np.inf, free, False), (0.0, 0.0 * free, True), (-0.5 * norm, -0.5 * free, True), (-2.0 * norm, free, False),
                              (0.5 * norm, 0.5 * free, True)):
        c = ctl.copy()
        c[:, phr.F_MAX] = value
        c64 = c.astype(np.float64)
        top = c64[:, phr.F_MAX]
        with np.errstate(invalid="ignore"):
            literal = (free * free).sum(axis=1) > top * top
        assert (literal == acts).all() and (phr.saturated(st, c)[0] == acts).all(), value
        got = phr.wrench(st, c)[:, 0:3]
        scaled = free * (top / norm)[:, None] if acts else free
        assert np.allclose(got, scaled, rtol=1e-12, atol=0) and np.allclose(got, want, rtol=1e-6, atol=1e-12), value


def test_the_control_poisons():
    st, pv, _, _ = mp.designed_population()
    rng = np.random.default_rng(6)
    n = 321
    ctl = phr.record(n, st[:, 0:3] + rng.normal(size=(n, 3)), rng.normal(size=(n, 4)), rng.uniform(1, 5, (n, 3)), rng.uniform(0, 1, (n, 3)), 2.0, 0.5)
    for size in vc.SIZES:
        bad, bodies, names = vc.poison_control(ctl, st, size)
        assert set(names) == {r[0] for r in vc.CONTROL_POISONS}
        others = ~np.isin(np.arange(size), bodies)
        assert vc.same_bits(bad[others], ctl[:size][others])
        b = bodies[names.index("f_max_negative")]
        assert bad[b, phr.F_MAX] < 0 and phr.saturated(st[:size], bad)[0][b]
        assert not phr.saturated(st[:size], bad)[0][bodies[names.index("f_max_nan")]]
        only, _, only_names = vc.poison_control(ctl, st, size, only=vc.F_MAX_ROWS)
        assert set(only_names) == set(vc.F_MAX_ROWS) and not np.isnan(np.delete(only, phr.F_MAX, axis=1)).any()


# ---- 2. the extremes fold ----------------------------------------------------------------------------------------------------------------
def _rows(n, steps=7, seed=11):
    """Rows and tensions with what a poisoned launch leaves in a log: NaN and +-Inf positions, overflowing speeds, exact zeros."""
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(steps, n, 13)).astype(np.float32)
    T = np.abs(rng.normal(size=(steps, n))).astype(np.float32) * (rng.uniform(size=(steps, n)) > 0.3)
    rows[:, vc.ZERO_BODIES, 0:2] = 0.0
    T[:, vc.ZERO_BODIES] = 0.0
    rows[2:, 0, 0], rows[:, 31, 2], rows[3:, 32, 2], rows[:, 63, 2] = np.nan, np.nan, np.inf, -np.inf
    rows[:, 128, 7], rows[4:, 159, 8], rows[:, 160, 9] = np.inf, 3e38, np.nan
    T[3, 70], T[5, 79] = np.inf, np.inf
    return rows, T


def _fold(rows, T, seed, lo=lambda x, m: np.where(x < m, x, m), hi=lambda x, m: np.where(x > m, x, m)):
    """Extremes.fold with the update given: the stand-in device of the mutation test."""
    rec = np.array(seed, np.float32)
    from silver2_isaacsim_amd.extremes import speed2
    with np.errstate(invalid="ignore"):
        for s, t in zip(rows, T):
            for a in range(3):
                rec[:, 2 * a], rec[:, 2 * a + 1] = lo(s[:, a], rec[:, 2 * a]), hi(s[:, a], rec[:, 2 * a + 1])
            rec[:, 6], rec[:, 7] = hi(speed2(s[:, 7:10]), rec[:, 6]), hi(t, rec[:, 7])
    return rec


def test_the_seed_and_the_fold_checker():
    for n in vc.SIZES:
        seed = vc.seeded_record(n)
        rows, T = _rows(n)
        counts = vc.assert_rows_cover(rows, T, seed)
        assert counts["neg_inf"] and counts["tension_inf"]
        for f in range(8):                                         # both NaNs in each of the eight fields, on bodies of their own
            assert vc.bits(seed[64 + 2 * f, f])[0] == 0x7fc01234 and vc.bits(seed[65 + 2 * f, f])[0] == 0xffc00000
        assert np.isnan(seed).sum() == 16 and (np.isnan(seed).sum(axis=1) <= 1).all()
        assert (seed[vc.HUGE_BODIES[0], [1, 7]] == np.float32(3e38)).all() and vc.same_bits(seed[5], Extremes.empty(1)[0])
        device = _fold(rows, T, seed)
        want = vc.check_extremes(device, rows, T, seed)
        # the fold keeps what the header says it keeps
        assert np.isnan(want[vc.NAN_SEED_BODIES, np.repeat(np.arange(8), 2)]).all()
        assert vc.same_bits(want[vc.NAN_SEED_BODIES, np.repeat(np.arange(8), 2)], seed[vc.NAN_SEED_BODIES, np.repeat(np.arange(8), 2)])
        assert np.signbit(want[vc.ZERO_BODIES[0], 0:4]).all() and not np.signbit(want[vc.ZERO_BODIES[1], 0:4]).any()
        assert np.signbit(want[vc.ZERO_BODIES[2], 7]) and want[70, 7] == np.inf
        assert not np.isnan(np.delete(want, [0, 31, 160], axis=0)[:, 0:6][~np.isnan(np.delete(seed, [0, 31, 160], axis=0)[:, 0:6])]).any()   # a NaN sample never enters
        # the mutation: fminf / fmaxf drop a NaN accumulator (and let -0 < +0 decide a tie)
        with pytest.raises(AssertionError):
            vc.check_extremes(_fold(rows, T, seed, lo=lambda x, m: np.fmin(m, x), hi=lambda x, m: np.fmax(m, x)), rows, T, seed)
        with pytest.raises(AssertionError):                        # rows without the ties are not this section's rows
            moved = rows.copy()
            moved[:, vc.ZERO_BODIES[0], 0] = 1e-30
            vc.assert_rows_cover(moved, T, seed)


def test_exact_zero_bodies_are_dry_upright_and_idle():
    st, pv, pr, moor = mp.designed_population()
    n = 321
    applied, ctl = np.ones((n, 6), np.float32), phr.record(n, st[:, 0:3] + 1, st[:, 3:7], 3.0, 1.0, 2.0, 0.5)
    s, p, a, c, m = vc.exact_zero_bodies(st, pv, applied, ctl, moor)
    z = vc.ZERO_BODIES
    assert not vc.bits(s[z, 0:2]).any() and (s[z, 2] >= 50).all() and (s[z, 2] - pr[z, 0:3].max(axis=1) > 10).all()
    assert not a[z].any() and not mr.has_line(m)[z].any() and not phr.wrench(s[z], c[z]).any()
    designed = np.array([*z, *vc.INF_BODIES, vc.INF_TENSION_BODY])
    others = ~np.isin(np.arange(n), designed)
    assert all(vc.same_bits(x[others], y[others]) for x, y in ((s, st), (p, pv), (a, applied), (c, ctl), (m, moor)))
    assert not np.isin(designed, vc.poisoned_bodies(200)).any() and not np.isin(designed, vc.poisoned_bodies(321)).any()
    assert s[vc.INF_BODIES[0], 0] == np.inf and s[vc.INF_BODIES[1], 1] == -np.inf and np.isinf(s).sum() == 2 and (s[list(vc.INF_BODIES), 2] >= 50).all()
    b = vc.INF_TENSION_BODY
    assert m[b, 7] == np.inf and mr.tension(moor, st)[b] > 0 and vc.same_bits(np.delete(m[b], 7), np.delete(moor[b], 7)) and vc.same_bits(s[b], st[b])


# ---- 3. malformed records ----------------------------------------------------------------------------------------------------------------
def test_the_conditions_on_the_tables(tethers, lines):
    """Every case of the issue's table is on a lane of its own; the fp64 reference and the fp32 emulation decide alike on every
    case lane; every finite stretch keeps its margin; the classes are those the checker is to meet."""
    st, _, rec, groups, tables = tethers
    ls, _, lrec, ltables = lines
    for family, state, tabs in (("tether", st, tables), ("mooring", ls, ltables)):
        fam = vc.FAMILIES[family]
        for n, t in tabs.items():
            names = [name for name, _ in t.cases]
            assert names == list(vc.CASES[family]), names
            bodies = [b for _, b in t.cases]
            # (a tether's NaN fairlead makes a case lane of its partner too: the partner's own wrench is formed from it)
            assert len(set(bodies)) == len(bodies) and t.lanes.sum() == len(bodies) + (family == "tether") and t.lanes[bodies].all()
            s = state[:n]
            _, _, pulls = vc.emulated(family, t.bad, s)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                pulls64 = fam.ref.tension(t.bad.astype(np.float64), s) > 0
                _, _, l, x, _, _ = fam.ref.geometry(t.bad.astype(np.float64), s)
            assert np.array_equal(pulls[t.lanes], pulls64[t.lanes]), (family, n)                    # no exclusions
            measured = t.lanes & fam.has(t.bad) & np.isfinite(x)
            assert measured.sum() >= 6 and (np.abs(x[measured]) >= vc.MARGIN * (l[measured] + np.abs(t.bad[measured, fam.L0]))).all(), (family, n)
            assert vc._decisive(family, t.bad, s, np.flatnonzero(t.lanes))
            for name, b in t.cases:
                assert name not in vc.MUST or t.kind[b] == vc.MUST[name], (family, n, name, t.kind[b])
            counts = {k: int((t.kind[t.lanes] == k).sum()) for k in ("pulls", "nothing", "non-finite")}
            assert counts["pulls"] >= (8 if family == "tether" else 3) and counts["nothing"] >= 6 and counts["non-finite"] == 2, (family, n, counts)
            # one malformation on one member: every other lane keeps the clean record
            assert vc.same_bits(np.delete(t.bad, bodies, axis=0), np.delete(t.clean, bodies, axis=0))
            print(f"[value contract, {family}, n = {n}] case lanes: {counts}  " + "  ".join(f"{name}:{b}" for name, b in t.cases))
    for n, t in tables.items():
        case = dict(t.cases)
        j, clean_j = tr.partner(t.bad), tr.partner(t.clean)
        dead = case[vc.DEAD]
        assert dead == n - 1 and j[dead] >= n and j[dead] // 64 == dead // 64 and t.kind[dead] == "pulls"     # (its margin: _decisive, above)
        assert j[case["partner_self"]] == case["partner_self"]
        a = case["partner_not_mutual"]
        assert j[a] != clean_j[a] and j[j[a]] != a and not t.lanes[j[a]] and tr.has_tether(t.bad)[j[a]]
        for name in ("partner_plus_64", "partner_minus_64", "partner_plus_0.7"):
            assert j[case[name]] == clean_j[case[name]] and t.bad[case[name], 6] != t.clean[case[name], 6], name
        assert j[case["partner_minus_0.5"]] % 64 == 0 and not t.lanes[j[case["partner_minus_0.5"]]]
        b = case["fairlead_nan"]
        assert t.lanes[clean_j[b]] and t.kind[clean_j[b]] == "nothing"
        assert t.structural.sum() == len(vc.STRUCTURAL) + 1 and (t.kind[t.structural] == "nothing").all()


def test_the_references_give_plus_zero_where_a_lane_adds_nothing(tethers, lines):
    """The fp64 wrench of both references is +0 for a lane that adds nothing, a NaN fairlead included (NaN x 0 is NaN)."""
    st, _, _, _, tables = tethers
    ls, _, _, ltables = lines
    for family, state, tabs in (("tether", st, tables), ("mooring", ls, ltables)):
        for n, t in tabs.items():
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                W = vc.FAMILIES[family].ref.wrench(t.bad.astype(np.float64), state[:n])
            idle = t.kind == "nothing"
            assert np.isnan(t.bad[idle]).any() and not W[idle].any() and not np.signbit(W[idle]).any(), (family, n)


def _stand_in(table, st, record):
    W, T, _ = vc.emulated(table.family, record, st[:len(record)])
    return W, (T if table.family == "tether" else None)


def _check(table, st, bad_device, bound=2.0):
    W, T = bad_device
    clean_W, clean_T = _stand_in(table, st, table.clean)
    return vc.check_probe(table, st, W, T, clean_W, clean_T, bound)


def test_the_probe_checker_passes_on_the_emulation_and_fails_on_its_mutations(tethers, lines, monkeypatch):
    st, _, rec, groups, tables = tethers
    ls, _, lrec, ltables = lines
    assert tr.PROBE_BOUND == mr.PROBE_BOUND == 2.0
    for family, state, tabs in (("tether", st, tables), ("mooring", ls, ltables)):
        fam = vc.FAMILIES[family]
        for n, t in tabs.items():
            figures = _check(t, state, _stand_in(t, state, t.bad), fam.ref.PROBE_BOUND)
            assert figures["worst"] <= fam.ref.PROBE_BOUND and figures["non_finite"] == 2
            print(f"[value contract, {family}, n = {n}] the emulation against fp64: {figures}")
            # "has a line" as not (k <= 0): the damper-only lane is no line any more
            with monkeypatch.context() as m:
                m.setitem(vc.FAMILIES, family, type(fam)(**{**vars(fam), "has": lambda r, fam=fam: ~(np.asarray(r)[:, fam.k] <= 0)}))
                m.setattr(fam.ref, "has_tether" if family == "tether" else "has_line", lambda r, fam=fam: ~(np.asarray(r)[:, fam.k] <= 0))
                mutant = _stand_in(t, state, t.bad)
            with pytest.raises(AssertionError, match=r"\(a\)"):
                _check(t, state, mutant)
            # +0 in place of a pull is caught, and so is a pull in place of +0
            W, T = _stand_in(t, state, t.bad)
            body = dict(t.cases)["k_nan_c_zero"]
            W = W.copy()
            W[body, 0] = -0.0
            with pytest.raises(AssertionError):
                _check(t, state, (W, T))
    for n, t in tables.items():
        case = dict(t.cases)
        # a dead partner that answers a non-zero value
        with monkeypatch.context() as m:
            def answering(r, a, answer=np.float32(1.0)):
                j = tr.partner(r)
                out = np.full_like(a, answer)
                out[j < len(a)] = a[j[j < len(a)]]
                return out
            m.setattr(tr, "_from_partner", answering)
            mutant = _stand_in(t, st, t.bad)
        with pytest.raises(AssertionError, match=r"\(c\)"):
            _check(t, st, mutant)
        # the partner modulo 64 after rounding to nearest: partner + 0.7 names the next lane
        with monkeypatch.context() as m:
            m.setattr(tr, "partner", lambda r: (np.arange(len(r)) // 64) * 64 + (np.rint(np.asarray(r)[:, 6]).astype(np.int64) & 63))
            mutant = _stand_in(t, st, t.bad)
        with pytest.raises(AssertionError, match=r"\(c\)|\(a\)"):
            _check(t, st, mutant)
        assert _check(t, st, _stand_in(t, st, t.bad))["pulls"] >= 5                                   # (the patches are gone)
        # (e): a well-formed lane that moves by one bit
        W, T = _stand_in(t, st, t.bad)
        lane = int(np.flatnonzero(~t.lanes & (t.kind == "pulls"))[0])
        W = W.copy()
        W[lane, 2] = np.nextafter(W[lane, 2], np.float32(np.inf))
        with pytest.raises(AssertionError, match=r"\(e\)"):
            _check(t, st, (W, T))


def test_plus_zero_added_to_an_untouched_wrench_is_seen(tethers):
    """In a step a lane that adds nothing leaves the wrench as it is: the wrench the step logs has the bits of the launch with that
    lane's k = c = 0.  A stand-in that adds W = +0 instead turns a component of -0 into +0, and the comparison of bits sees it."""
    st, _, _, _, tables = tethers
    t = tables[200]
    W, _, pulls = vc.emulated("tether", t.bad, st[:200])
    Wn, _, pulls_n = vc.emulated("tether", vc.neutralised(t, t.kind == "nothing"), st[:200])
    assert np.array_equal(pulls, pulls_n)
    rng = np.random.default_rng(3)
    f6 = rng.normal(size=(200, 6)).astype(np.float32)
    f6[:, 1] = -0.0                                                # (a dry or symmetric body: a component of exactly -0)
    keeps = lambda f, w, p: np.where(p[:, None], f + w, f)  # noqa: E731
    adds = lambda f, w, p: f + np.where(p[:, None], w, np.float32(0))  # noqa: E731
    vc.assert_same_bits(keeps(f6, W, pulls), keeps(f6, Wn, pulls_n))
    with pytest.raises(AssertionError):
        vc.assert_same_bits(adds(f6, W, pulls), keeps(f6, Wn, pulls_n))


def test_the_peak_checker_takes_an_infinite_sample():
    rng = np.random.default_rng(9)
    samples = np.abs(rng.normal(size=(7, 4, 200))).astype(np.float32) * (rng.uniform(size=(7, 4, 200)) > 0.5)
    samples[3, 0, 17] = np.inf
    peaks = samples.max(axis=0).T.copy()
    vc.check_peaks(peaks, samples)
    assert peaks[17, 0] == np.inf
    peaks[17, 0] = np.float32(3e38)
    with pytest.raises(AssertionError):
        vc.check_peaks(peaks, samples)
