"""tests/statistics_contract.py shown on the host: the tables are what they claim, each of the six mutations of `fold` fails
`check_record`, and - the finding this module exists for - with the levels tests/test_statistics_gpu.py takes (the initial value
+- 1e-3, 0, 50 N, the mean) the fused and the fp32-difference mutations give `fold`'s bits on EVERY body: a bit comparison on those
levels cannot see a contracted fma or a narrowed subtraction.  The conditions on the inputs (statistics_contract's caps) are asserted
here on the fp64 closed loop's samples, rounded to fp32, and again by the GPU tests on the device's own rows.

Samples: (a) closed_loop_reference.closed_loop over the first 200 bodies of the moored designed population in a current, implicit
drag, 7 steps; (b) the same with value_contract's designed bodies - exact zeros, +-Inf positions, a +Inf tension, the poison table -,
which supply every meeting of `assert_rows_cover` but a finite sample after a NaN one: on the host that one is made by healing the
poisoned bodies after the third step, as the GPU test does between its launches of 3 and 4 steps."""
import os

import numpy as np
import pytest

import mooring_population as mp
import statistics_contract as sc
import value_contract as vc
from closed_loop_reference import closed_loop
from conftest import REPO
from populations import DT, G, RHO
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.sea import SeaState

N, STEPS = 200, 7
CURRENT = SeaState((0.5, -0.2, 0.05))
PAIRS = ((0, 6), (1, 5), (2, 2))                                   # (x, tension), (y, vz), (z, z)


def _run(st, pv, pr, moor, steps):
    with np.errstate(all="ignore"):
        out = closed_loop(st, pv, pr, RHO, G, DT, steps, sea=CURRENT, moor=moor, implicit=True)
    rows = np.stack([np.asarray(s["state"], np.float32) for s in out])
    with np.errstate(invalid="ignore"):
        T = np.stack([np.where(s["tension"] > 0, s["tension"], 0.0).astype(np.float32) for s in out])
    return rows, T


@pytest.fixture(scope="module")
def clean():
    """(rows (7, n, 13), T (7, n)) of the moored designed population."""
    st, pv, pr, moor = (a[:N] for a in mp.designed_population())
    return (st, *_run(st, pv, pr, moor, STEPS))


@pytest.fixture(scope="module")
def designed():
    """The same with the exact-zero bodies, the bodies at infinity and the poison table; the poisoned bodies healed after step 3."""
    st, pv, pr, moor = (a[:N] for a in mp.designed_population())
    zst, zpv, _, _, zmoor = vc.exact_zero_bodies(st, pv, np.zeros((N, 6), np.float32), np.zeros((N, 17), np.float32), moor)
    zst = sc.more_infinities(zst)
    ps, pp, bodies, _ = vc.poison(zst, zpv, N)
    rows3, T3 = _run(ps, pp, pr, zmoor, 3)
    healed, prev = rows3[-1].copy(), rows3[-2][:, 7:13].copy()     # (the previous velocity: that of the state the last step started from)
    healed[bodies], prev[bodies] = zst[bodies], zpv[bodies]
    rows4, T4 = _run(healed, prev, pr, zmoor, 4)
    return np.concatenate([rows3, rows4]), np.concatenate([T3, T4]), bodies


def _samples(rows, T, pair):
    return stx.samples_of(rows, T, pair[0]), stx.samples_of(rows, T, pair[1])


def test_the_header_says_what_the_tables_hold_it_to():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    for phrase in ("n is a uint32_t and\n * wraps modulo 2^32", "it is never above, so it leaves bit 31\n * set and the next sample above the level counts",
                   "(modulo 2^31)", "x == L is not above", "a NaN or infinite level poisons that body's slot", "NO fused multiply-add anywhere"):
        assert phrase in text, phrase


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_gap_levels_lie_five_to_twelve_orders_below_with_a_full_mantissa(clean):
    _, rows, T = clean
    for pair in PAIRS:
        a, b = _samples(rows, T, pair)
        s0 = np.stack([a[0], sc.first_nonzero(b)], axis=1)
        lev = sc.gap_levels(s0, 5)
        assert lev.dtype == np.float32 and lev.shape == (N, 2) and np.isfinite(lev).all() and (lev != 0).all()
        assert (lev.view(np.uint32) & 1).all()                     # the mantissa's last bit: nothing of it is short
        below = sc.orders_below(s0, lev)
        usable = np.isfinite(s0) & (np.abs(s0) > 1e-30)
        assert ((below[usable] >= 5) & (below[usable] <= 12)).all() and set(np.unique(below[usable])) == set(range(5, 13))
        assert (lev[~usable] == sc.FALLBACK_LEVEL).all()
        assert np.array_equal(lev, sc.gap_levels(s0, 5)) and not np.array_equal(lev, sc.gap_levels(s0, 6))
    odd = sc.gap_levels(np.array([[0.0, np.nan], [np.inf, -np.inf], [1e-44, -0.0]], np.float32), 1)
    assert (odd == sc.FALLBACK_LEVEL).all() and sc.FALLBACK_LEVEL.view(np.uint32) & 1


def test_the_level_table_is_what_it_claims(designed):
    rows, T, _ = designed
    for pair in PAIRS:
        a, b = _samples(rows, T, pair)
        lev, names = sc.level_table(a, b, 11, zero_bodies=sc.ZERO_BODIES)
        dealt = (names != "").any(axis=1)
        assert dealt.mean() <= sc.LEVEL_ROWS_CAP and set(sc.LEVEL_ROWS) <= set(names.ravel())
        assert set(names[sc.ZERO_BODIES].ravel()) == {"-0", "+0"}
        gap = sc.gap_levels(np.stack([a[0], b[0]], axis=1), 11)
        assert np.array_equal(lev[names == ""].view(np.uint32), gap[names == ""].view(np.uint32))
        lanes = np.flatnonzero(dealt) % 64
        assert {0, 31, 32, 63} <= set(lanes.tolist()) and dealt[N - 1] and dealt[64 * ((N - 1) // 64)]
        for c, xs in enumerate((a, b)):
            for body in np.flatnonzero(names[:, c] == "sample"):
                assert vc.same_bits(lev[body, c], xs[body % STEPS, body])
            for body in np.flatnonzero(names[:, c] == "sample_up"):
                x = xs[body % STEPS, body]
                assert np.isnan(x) or lev[body, c] > x or np.isposinf(x)
            assert np.isnan(lev[names[:, c] == "nan", c]).all() and np.isposinf(lev[names[:, c] == "+inf", c]).all()
            assert (lev[names[:, c] == "denormal", c].view(np.uint32) == 1).all() and (lev[names[:, c] == "-denormal", c].view(np.uint32) == 0x80000001).all()
            assert (np.abs(lev[np.isin(names[:, c], ("+3e38", "-3e38")), c]) == np.float32(3e38)).all()


def test_the_seeded_record_is_what_it_claims(clean):
    _, rows, T = clean
    a, b = _samples(rows, T, PAIRS[1])
    seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 3)
    sums = seed["sums"]
    assert sums.dtype == np.float64 and seed["up"].dtype == np.uint32 and seed["n"].dtype == np.uint32
    bits = sums.view(np.uint64)
    for want in (0x8000000000000000, 0x7ff8000000001234, 0xfff8000000000000, 0x7ff0000000000000, 0xfff0000000000000, np.array([1e300]).view(np.uint64)[0]):
        assert (bits == np.uint64(want)).any(), hex(want)
    assert set(sc.UP_SEEDS) <= set(seed["up"][:, 0].tolist()) and set(sc.UP_SEEDS) <= set(seed["up"][:, 1].tolist())
    assert set(sc.N_SEEDS) <= set(seed["n"].tolist())
    full = sc.full_mantissa_bodies(N)
    assert full.sum() >= N // 10 and np.isfinite(sums[full]).all() and (sums[full] != 0).all()
    assert (bits[full] & np.uint64(0xfffff)).all(axis=1).mean() > 0.9      # (nothing short about them)
    ratio = np.abs(sums[full][:, [0, 2]]) / np.abs(np.stack([a[0], b[0]], axis=1)[full].astype(np.float64))
    assert ((ratio >= 1) & (ratio < 2)).any() and ((ratio >= 2.0 ** 40) & (ratio < 2.0 ** 41)).any()
    untouched = (np.arange(N) % 3 != 1)
    assert not bits[untouched].any()
    assert sc.same_record(stx.fold(seed, a[:0], b[:0], np.zeros((N, 2), np.float32)), seed)      # fold takes a seed as it is


def test_the_restatement_is_fold(clean, designed):
    for rows, T in (clean[1:], designed[:2]):
        for pair in PAIRS:
            a, b = _samples(rows, T, pair)
            lev, _ = sc.level_table(a, b, 2, zero_bodies=sc.ZERO_BODIES)
            seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
            for record in (None, seed):
                assert sc.same_record(sc.fold_restated(record, a, b, lev), stx.fold(record, a, b, lev))
            three = stx.fold(seed, a[:3], b[:3], lev)
            assert sc.same_record(stx.fold(three, a[3:], b[3:], lev), stx.fold(seed, a, b, lev))       # 3 + 4 is 7, n's wrap included


def test_the_designed_samples_hold_every_meeting(designed):
    rows, T, _ = designed
    total = dict.fromkeys(sc.MEETINGS, 0)
    for pair, absent in zip(PAIRS, (("-inf_finite_level", "-inf_same_infinity"), ("+inf_finite_level", "+inf_same_infinity"),
                                    ("+inf_finite_level", "+inf_same_infinity", "-inf_finite_level", "-inf_same_infinity", "+0_against_-0"))):
        a, b = _samples(rows, T, pair)
        lev, _ = sc.level_table(a, b, 2, zero_bodies=sc.ZERO_BODIES)
        seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
        counts = sc.assert_rows_cover(a, b, lev, seed, require=[m for m in sc.MEETINGS if m not in absent])
        for k, v in counts.items():
            total[k] += v
        want = sc.check_record(stx.fold(seed, a, b, lev), a, b, lev, seed)
        # what the header says of these meetings, read off fold's record
        nan_then_finite = np.isnan(a).any(axis=0) & np.isfinite(a[-1]) & np.isfinite(lev[:, 0])
        assert nan_then_finite.any() and np.isnan(want["sums"][nan_then_finite, 0:2]).all()          # NaN for good
        wrapped = (seed["up"][:, 0] == 0xffffffff) & (a[0] > lev[:, 0])
        assert wrapped.any() and ((stx.fold(seed, a[:1], b[:1], lev)["up"][wrapped, 0]) == 0).all()  # the count wraps to 0, bit 31 clears
        assert (want["n"][seed["n"] == 0xffffffff] == 6).all() and (want["n"][seed["n"] == 0xfffffffd] == 4).all()
    assert all(total.values()), total
    with pytest.raises(AssertionError):
        a, b = _samples(rows, T, PAIRS[2])
        sc.assert_rows_cover(a, b, sc.gap_levels(np.stack([a[0], b[0]], axis=1), 1), stx.empty(N))


# ---- the mutations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.MUTATIONS))
def test_each_mutation_fails_check_record(name, designed):
    """The record a device with that mistake would leave, over the designed samples from the seeded record: check_record refuses it
    on at least one channel pair - and accepts fold's own."""
    rows, T, _ = designed
    refused = 0
    for pair in PAIRS:
        a, b = _samples(rows, T, pair)
        lev, _ = sc.level_table(a, b, 2, zero_bodies=sc.ZERO_BODIES)
        seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
        sc.check_record(stx.fold(seed, a, b, lev), a, b, lev, seed)
        got = sc.MUTATIONS[name](seed, a, b, lev)
        try:
            sc.check_record(got, a, b, lev, seed, name)
        except AssertionError:
            refused += 1
            with pytest.raises(AssertionError):                    # the other way round: fold's record against the mutation as the rule
                sc.check_record(stx.fold(seed, a, b, lev), a, b, lev, seed, name, fold=sc.MUTATIONS[name])
    assert refused >= 1, name
    if name in ("fused", "fp32_difference", "pairwise"):
        assert refused == len(PAIRS), name


# ---- the finding --------------------------------------------------------------------------------------------------------------------------
def _present_levels(st, rows, T, pair, seed):
    """The levels tests/test_statistics_gpu.py takes: a motion or velocity channel's initial value - 1e-3, + 0 or + 1e-3
    (its _levels_for), 50 N in slot a and +0 in slot b on the tension; exactly 0; and the fp64 mean of the rows
    (statistics_reference.levels_of)."""
    rng = np.random.default_rng(seed)
    a, b = _samples(rows, T, pair)
    near = np.stack([np.zeros(N, np.float32) if c == 6 else st[:, stx.STATE_FIELD[c]] for c in pair], axis=1).astype(np.float32)
    near = (near + rng.choice(np.array([-1e-3, 0.0, 1e-3], np.float32), size=near.shape)).astype(np.float32)
    for c, ch in enumerate(pair):
        if ch == 6:
            near[:, c] = (50.0, 0.0)[c]
    mean = np.stack([a.astype(np.float64).mean(axis=0), b.astype(np.float64).mean(axis=0)], axis=1).astype(np.float32)
    return {"the initial value +- 1e-3, 50 N, +0": near, "zero": np.zeros((N, 2), np.float32), "the mean of the rows": mean}


def test_the_present_levels_have_no_teeth(clean):
    """With the levels the GPU tests took before this module a fused S2 and an fp32 difference are fold's bits on every body (but one in 1 600, whose coordinate is itself of the order of
    1e-3) of every position channel (the initial value +- 1e-3: Sterbenz, and a d of few bits), of the tension (50 N, +0) and of any channel
    against exactly 0: there the comparison could not fail for either mistake.  Only a velocity channel against its initial value
    +- 1e-3 could see them - a velocity moves by far more than 1e-3 in a step -: on the reference's vz a fused S2 differs on about
    18 % of the bodies and an fp32 difference on about 85 % (printed, with the figures for the mean of the rows; asserted to be
    there, so that this docstring stays true).  Do not go back to those levels for this purpose."""
    st, rows, T = clean
    compared, seen, exceptions = 0, {}, 0
    for i, pair in enumerate(PAIRS):
        a, b = _samples(rows, T, pair)
        for kind, lev in _present_levels(st, rows, T, pair, 100 + i).items():
            want = stx.fold(None, a, b, lev)
            finite = sc.finite_pairs(a, b, lev)
            fused = sc.s2_differs(sc.fold_fused(None, a, b, lev), want) & finite
            narrow = sc.s2_differs(sc.fold_fp32_difference(None, a, b, lev), want) & finite
            for c, ch in enumerate(pair):
                print(f"[present levels, channel {stx.CHANNELS[ch]} in slot {'ab'[c]}, {kind}] S2 differs on {fused[:, c].mean():.3f} (fused) and "
                      f"{narrow[:, c].mean():.3f} (fp32 difference) of {finite[:, c].sum()} bodies")
                if kind == "zero" or (kind != "the mean of the rows" and ch in (0, 1, 2, 6)):
                    compared += int(finite[:, c].sum())
                    assert fused[:, c].mean() <= 0.01 and narrow[:, c].mean() <= 0.01, (ch, kind, fused[:, c].mean(), narrow[:, c].mean())
                    exceptions += int(fused[:, c].sum() + narrow[:, c].sum())
                elif kind != "the mean of the rows":
                    seen[ch] = (fused[:, c].mean(), narrow[:, c].mean())
    assert exceptions <= 2, exceptions                             # (a body whose coordinate is itself of the order of 1e-3)
    assert compared >= 8 * N and seen and all(f > 0 and w > 0 for f, w in seen.values()), (compared, seen)


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------------------
def test_the_caps_hold_on_the_reference(clean, designed):
    st, rows, T = clean
    for i, pair in enumerate(PAIRS):
        a, b = _samples(rows, T, pair)
        lev = sc.gap_levels(np.stack([sc.first_nonzero(a), sc.first_nonzero(b)], axis=1), 40 + i)
        figures = sc.assert_gap_caps(a, b, lev, pair)
        print(f"[gap levels, one draw, channels {pair}, 7 steps from the empty record] {figures}")
        lev = sc.designed_gap_levels(a, b, 40 + i)
        below = sc.orders_below(np.stack([sc.first_nonzero(a), sc.first_nonzero(b)], axis=1), lev)
        assert ((below >= 5) & (below <= 12))[np.isfinite(below)].all() and (lev.view(np.uint32) & 1).all()
        figures = sc.assert_gap_caps(a, b, lev, pair)
        assert figures["fused"] >= 0.5, figures                    # (of four draws the first that shows: 1 - 0.7^4 if the draws were all)
        print(f"[gap levels, designed, channels {pair}, 7 steps from the empty record] {figures}")
        seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
        print(f"[seeded record, channels {pair}] {sc.assert_seeded_caps(a, b, lev, seed, pair)}")
    rows, T, _ = designed
    for pair in PAIRS:
        a, b = _samples(rows, T, pair)
        lev, _ = sc.level_table(a, b, 2, zero_bodies=sc.ZERO_BODIES)
        seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
        print(f"[seeded record, designed samples, channels {pair}] {sc.assert_seeded_caps(a, b, lev, seed, pair)}")
