"""The value rules of include/hydro.h, "Statistics", on the device, at inputs where breaking them changes a bit: the tables and
checkers are tests/statistics_contract.py's (shown on the host by tests/test_statistics_contract.py, where each of six mutations of
`fold` fails `check_record`), the launches are made here through resident_harness.step.  Every comparison is equality of bits with
`statistics.fold`; the CONDITIONS on the inputs (statistics_contract's caps: a fused S2 would differ on a quarter of the finite pairs,
an fp32 difference on half, a pairwise sum and a fused S2 on a quarter of the full-mantissa seeds) are asserted on the device's own
rows BEFORE the comparison, so a launch whose samples could not tell the mistakes apart fails instead of passing.

1. GAP LEVELS, EVERY CHANNEL: the launch of tests/test_statistics_gpu.py's motion test (sea, bed, a line, applied wrench, pose hold,
   every body recorded), 7 steps and 3 + 4, each of X .. VZ in slot a and in slot b; the tension over seven one-step launches.
2. THE SEEDED FOLD WITH DESIGNED SAMPLES: value_contract's exact-zero bodies, bodies at x = +Inf and y = -Inf (two of each: one
   meets a finite level, one its own infinity), a +Inf tension and the poison table, in a current; the level table and the seeded
   record; 7 steps at once and as 3 + 4, where the poisoned bodies are healed between the two launches so that finite samples follow
   NaN ones; channel pairs (x, tension), (y, vz), (z, z).  `assert_rows_cover` asserts every meeting; the counts are printed.
3. THE TENSION ABOVE ONE LAYER: spreads of three and four layers in still water, the regular sea and spectra of 11 and 64
   components; channels (tension, tension) against (gap, +0) equal `fold` over the seven tension_max.
4. SIZES WITHOUT A TAIL AND WITH MANY BLOCKS: n = 1, 64, 256 and 4097; the padding lanes keep the NaN they were created with.
5. ISOLATION: the poison table in the state leaves every other body's words those of the clean launch.

WHY NO VALUE IN A STATE, A LEVEL OR A RECORD CAN FORM AN ADDRESS OR A LOOP BOUND (read in silver2_isaacsim_amd/csrc/hydro_kernels.hip
before the first run; tests/test_value_contract_gpu.py states the same for everything below the statistics).  StatisticsTrack::begin
forms `tile_lev` and `tile_stat` from the tile index and the host-validated strides, and every load and store of the two records is
`at<>(r, lane4, constant)`: tile, lane and a constant.  The parked sums live in LDS at lane4 + a wave offset from threadIdx.  `fold`
uses x, L and the words as VALUES only (a subtraction, two additions, a product, a compare, integer arithmetic on the word); `sample`
picks a channel by compares with `channel_a` / `channel_b`, kernel arguments the host validated to 0 .. 6.  `end` adds `steps`, a
host-validated argument, to the n word.  The loops run over `steps`, `layers` and `waves`.  So a NaN, an infinity or 0xffffffff in a
level or a seeded record selects no address and bounds no loop: these tests provoke nothing.

Sizes: n = 200 and 321 (test 4: 1, 64, 256, 4097); f32 and f16 coefficient records; explicit and implicit drag where the samples stay
finite without a pose hold.  One engine per (n, coefficient format) serves the module.  The figures of an MI355X are in DESIGN.md
section 30."""
import numpy as np
import pytest
import torch

import mooring_spread_reference as msr
import populations
import sea_spectrum_reference as ssr
import statistics_contract as sc
import value_contract as vc
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.sea import SeaSpectrum
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import moored_pop  # noqa: F401  (a fixture)
from resident_harness import _buffers, COEFFS, DEV, DRAG, _engine, _from, _log, NAN, _rows, step, _tiled
from statistics_reference import live_words
from value_contract_launches import CURRENT, engines, pop  # noqa: F401  (pop, engines: fixtures)

pytestmark = pytest.mark.gpu
SIZES = (200, 321)
PAIRS = ((0, 3), (1, 4), (2, 5), (3, 0), (4, 1), (5, 2))          # each of X .. VZ in slot a and in slot b
DESIGNED_PAIRS = ((0, 6), (1, 5), (2, 2))                          # (x, tension), (y, vz), (z, z)
CHUNKS = ([7], [3, 4])
FULL = ssr.designed_spectrum()
WATERS = {"still": None, "sea": SEA, "irr11": ssr.truncated(FULL, 11), "irr64": FULL}
INF = ("+inf_finite_level", "+inf_same_infinity", "-inf_finite_level", "-inf_same_infinity")
# what a channel pair of the designed population cannot hold: (x, tension) no -Inf, (y, vz) no +Inf, (z, z) neither, nor a +0
ABSENT = {(0, 6): INF[2:], (1, 5): INF[:2], (2, 2): INF + ("+0_against_-0",)}


def _record(eng, n, seed=None):
    """A record on the device: NaN everywhere and then reset, or `seed` (the dict of statistics.empty) with NaN in the padding lanes."""
    if seed is None:
        return eng.statistics_reset(torch.full((eng.tiles(n), nat.STAT_FIELDS, 64), NAN, dtype=torch.float32, device=DEV), n)
    host = stx.pack(seed, eng.tiles(n))
    words = host.reshape(host.shape[0], -1).view(np.uint32)
    words[~live_words(n, 704)] = 0x7FC00000
    return torch.from_numpy(host).to(DEV)


def _host(record, n):
    return stx.unpack(record.cpu().numpy(), n)


def _padding_is_nan(record, n):
    words = record.cpu().numpy().reshape(record.shape[0], -1).view(np.uint32)
    return bool((words[~live_words(n, 704)] == 0x7FC00000).all())


def _set_water(eng, water):
    eng.set_sea_spectrum(None)
    eng.set_sea(None)
    if isinstance(water, SeaSpectrum):
        eng.set_sea_spectrum(water)
    elif water is not None:
        eng.set_sea(water)


def _launches(eng, st, pv, n, chunks, implicit, *, record=None, levels=None, channels=None, step0=3, heal=None, **kw):
    """The launches of `chunks` steps through the _stat entry with every body recorded: (rows (steps, n, 13), the final state).
    heal = (bodies, state, prev): between the launches those bodies get that state and previous velocity."""
    cur, old = _buffers(st, pv, n)
    logs, done = [], 0
    for i, k in enumerate(chunks):
        if i and heal is not None:
            cur, old = _heal(cur, old, n, *heal)
        log = _log(k, n)
        step(eng, "stat", cur, old, n, k, step0=step0 + done, statistics=record, levels=None if record is None else _tiled(levels), channels=channels,
             implicit=implicit, log=log, **kw)
        cur, old = old, cur
        logs.append(_rows(log)[:, :, :13])
        done += k
    torch.cuda.synchronize()
    return np.concatenate(logs), _from(cur, n)


def _heal(cur, old, n, bodies, st, pv):
    c, o = _from(cur, n), _from(old, n)
    c[bodies], o[bodies, 7:13] = st[bodies], pv[bodies]
    return _tiled(c), _tiled(o)


def _tension_chain(eng, st, pv, n, implicit, *, record=None, levels=None, channels=(6, 6), step0=3, heal=None, heal_at=3, **kw):
    """Seven one-step launches, each with an extremes record reset to empty, so that tension_max of each is that step's sample:
    (rows (7, n, 13), T (7, n))."""
    cur, old = _buffers(st, pv, n)
    rows, T = [], []
    for k in range(7):
        if k == heal_at and heal is not None:
            cur, old = _heal(cur, old, n, *heal)
        one, log = _tiled(ex.Extremes.empty(n)), _log(1, n)
        step(eng, "stat", cur, old, n, 1, step0=step0 + k, statistics=record, levels=None if record is None else _tiled(levels),
             channels=channels if record is not None else None, extremes=one, implicit=implicit, log=log, **kw)
        cur, old = old, cur
        torch.cuda.synchronize()
        rows.append(_rows(log)[0, :, :13])
        T.append(_from(one, n)[:, 7])
    return np.stack(rows), np.stack(T)


def _pooled(parts):
    """[(samples_a, samples_b, levels)] side by side, as one launch of the sum of the bodies."""
    return tuple(np.concatenate([p[i] for p in parts], axis=0 if i == 2 else 1) for i in range(3))


# ---- 1. gap levels, every channel ---------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_motion_and_velocity_channels_with_gap_levels(coeff, implicit, moored_pop, engines):  # noqa: F811
    """A first launch without a record gives the rows; the levels lie 5 to 12 orders below each channel's first sample; the caps hold
    on those rows, pooled over the six channel pairs (the figures are printed); then every word of the record of the same launch, 7
    steps and 3 + 4, is fold of the rows."""
    st, pv, _, applied, ctl, rec = moored_pop
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        kw = dict(mooring=_tiled(rec[:n]), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]))
        rows, final = _launches(eng, st, pv, n, [7], implicit, **kw)
        parts = []
        for i, pair in enumerate(PAIRS):
            a, b = stx.samples_of(rows, None, pair[0]), stx.samples_of(rows, None, pair[1])
            parts.append((a, b, sc.designed_gap_levels(a, b, 100 * n + i)))
        figures = sc.assert_gap_caps(*_pooled(parts), (n, coeff, implicit))
        print(f"[gap levels, n = {n}, {coeff}, {'implicit' if implicit else 'explicit'}] over the six channel pairs: {figures}")
        for pair, (a, b, lev) in zip(PAIRS, parts):
            for chunks in CHUNKS:
                record = _record(eng, n)
                again, state = _launches(eng, st, pv, n, chunks, implicit, record=record, levels=lev, channels=pair, **kw)
                vc.assert_same_bits(again, rows, (n, pair, chunks, "rows"))
                vc.assert_same_bits(state, final, (n, pair, chunks, "nothing feeds back"))
                got = _host(record, n)
                sc.check_record(got, a, b, lev, None, (n, pair, chunks))
                assert (got["n"] == 7).all() and _padding_is_nan(record, n)


@COEFFS
@DRAG
def test_the_tension_channel_with_gap_levels(coeff, implicit, moored_pop, engines):  # noqa: F811
    """Seven one-step launches as in tests/test_statistics_gpu.py; the levels of both slots lie 5 to 12 orders below the body's first
    non-zero tension (the fallback level where its line never pulls).  As there, the sums are compared for the bodies that stay finite."""
    st, pv, _, _, _, rec = moored_pop
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        lines = _tiled(rec[:n])
        rows, T = _tension_chain(eng, st, pv, n, implicit, mooring=lines)
        first = sc.first_nonzero(T)
        lev = sc.designed_gap_levels(T, T, 7 * n)
        finite = np.isfinite(rows).all(axis=(0, 2)) & np.isfinite(st[:n]).all(axis=1)
        assert finite.mean() >= 0.98 if implicit else finite.any(), n
        taut = first > 0
        below = sc.orders_below(np.stack([first, first], axis=1), lev)[taut]
        assert taut.sum() >= (n // 5 if implicit else 1) and ((below >= 5) & (below <= 12)).all() and (lev != 0).all()
        figures = sc.assert_gap_caps(T[:, finite], T[:, finite], lev[finite], (n, coeff, implicit), least=64 if implicit else 8)
        print(f"[gap levels, tension, n = {n}, {coeff}, {'implicit' if implicit else 'explicit'}] {figures}")
        record = _record(eng, n)
        rows2, T2 = _tension_chain(eng, st, pv, n, implicit, record=record, levels=lev, mooring=lines)
        vc.assert_same_bits(rows2, rows, n)
        vc.assert_same_bits(T2, T, n)
        got = _host(record, n)
        assert (got["n"] == 7).all()
        sc.check_record({k: v[finite] for k, v in got.items()}, T[:, finite], T[:, finite], lev[finite], None, n)


# ---- 2. the seeded fold with designed samples -----------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_the_seeded_fold_with_designed_samples(coeff, implicit, pop, engines):  # noqa: F811
    z = pop["zero"]
    zst = sc.more_infinities(z["st"])
    total = dict.fromkeys(sc.MEETINGS, 0)
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_sea(CURRENT)
        eng.set_watch(list(range(n)))
        ps, pp, bodies, _ = vc.poison(zst, z["pv"], n)
        lines = _tiled(z["moor"][:n])
        for chunks in CHUNKS:
            heal = (bodies, zst, z["pv"]) if len(chunks) > 1 else None
            # the launch without a record: its rows, and the tensions of the chain of single steps, whose states are the launch's
            rows, _ = _launches(eng, ps, pp, n, chunks, implicit, heal=heal, mooring=lines)
            chain, T = _tension_chain(eng, ps, pp, n, implicit, heal=heal, heal_at=chunks[0], mooring=lines)
            vc.assert_same_bits(chain, rows, (n, chunks, "seven steps are seven single steps"))
            for pair in DESIGNED_PAIRS:
                a, b = stx.samples_of(rows, T, pair[0]), stx.samples_of(rows, T, pair[1])
                lev, _ = sc.level_table(a, b, 2, zero_bodies=sc.ZERO_BODIES)
                seed = sc.seeded_record(np.stack([a[0], b[0]], axis=1), 4)
                absent = ABSENT[pair] + (("finite_after_nan",) if heal is None else ())
                counts = sc.assert_rows_cover(a, b, lev, seed, require=[m for m in sc.MEETINGS if m not in absent])
                caps = sc.assert_seeded_caps(a, b, lev, seed, (n, pair, chunks))
                print(f"[seeded fold, n = {n}, {coeff}, {'implicit' if implicit else 'explicit'}, {chunks}, channels {pair}] {counts} {caps}")
                for k, v in counts.items():
                    total[k] += v
                record = _record(eng, n, seed)
                again, _ = _launches(eng, ps, pp, n, chunks, implicit, record=record, levels=lev, channels=pair, heal=heal, mooring=lines)
                vc.assert_same_bits(again, rows, (n, pair, chunks, "rows"))
                got = _host(record, n)
                sc.check_record(got, a, b, lev, seed, (n, pair, chunks))
                assert _padding_is_nan(record, n)
                # a NaN sample leaves bit 31 set: where the last sample is a NaN the word says "not above"
                for c, xs in enumerate((a, b)):
                    assert (got["up"][np.isnan(xs[-1]), c] >> 31).all()
    assert all(total.values()), total


# ---- 3. the tension above one layer, under every water ------------------------------------------------------------------------------------------
@COEFFS
@pytest.mark.parametrize("water", list(WATERS))
def test_the_largest_tension_of_a_spread_under_every_water(water, coeff, pop, engines):  # noqa: F811
    """Channels (tension, tension) against levels (gap, +0) over seven one-step launches with a spread of three and of four layers:
    fold over the seven tension_max of an extremes record reset to empty before each step.  Implicit drag (without a pose hold the
    explicit form leaves the fp32 range).  One body in eight at least has two layers taut in one step - by the fp64 reference at
    the initial state, and again at the state the device's first step produced."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = engines(n, coeff)
        _set_water(eng, WATERS[water])
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        for layers in (3, 4):
            sp = pop["spread"][:n, 0:9 * layers]
            T0 = msr.tensions(sp, np.asarray(st[:n], np.float64))
            assert ((T0 > 0).sum(axis=0) >= 2).mean() >= 1 / 8, (n, layers)
            kw = dict(mooring=_tiled(sp), mooring_layers=layers)
            _, first = _tension_chain(eng, st, pv, n, True, **kw)  # (the tensions, for the levels: the chain is repeated with the record)
            lev = sc.designed_gap_levels(first, first, 31 * n + layers)
            lev[:, 1] = 0.0
            record = _record(eng, n)
            rows, T = _tension_chain(eng, st, pv, n, True, record=record, levels=lev, **kw)
            vc.assert_same_bits(T, first, (n, layers, "the chain repeats"))
            T1 = msr.tensions(sp, rows[0].astype(np.float64))
            assert ((T1 > 0).sum(axis=0) >= 2).mean() >= 1 / 8, (n, layers, "on the device's rows")
            # the sample IS the largest: where the reference's largest is clear of the second by a factor of 1.5, the device's follows it
            top, second = np.sort(T0, axis=0)[-1], np.sort(T0, axis=0)[-2]
            clear = (top > 1.5 * second) & (second > 0)
            assert clear.sum() >= n // 16 and np.allclose(T[0][clear], top[clear], rtol=1e-3), (n, layers)
            finite = np.isfinite(rows).all(axis=(0, 2))
            assert finite.mean() >= 0.98, (n, layers, finite.mean())
            figures = sc.assert_gap_caps(T[:, finite], np.zeros_like(T[:, finite]), np.stack([lev[finite, 0], lev[finite, 0]], axis=1), (n, layers, water))
            print(f"[tension of {layers} layers, {water}, n = {n}, {coeff}] taut in two layers or more: {((T1 > 0).sum(axis=0) >= 2).mean():.3f} of the bodies; slot a: {figures}")
            got = _host(record, n)
            assert (got["n"] == 7).all()
            sc.check_record({k: v[finite] for k, v in got.items()}, T[:, finite], T[:, finite], lev[finite], None, (n, layers, water))
        eng.set_sea_spectrum(None)


# ---- 4. sizes without a tail and with many blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 256, 4097])
def test_sizes_without_a_tail_and_with_many_blocks(n, native_built):
    """7 steps, f32, implicit drag, a spectrum of 9 components, channels (x, vz), gap levels, every body recorded; the first n bodies of
    the integrator tests' population."""
    st, pv, pr = populations.integrator_population(n=4097, seed=31)
    eng = _engine(n, pr, "f32")
    eng.set_sea_spectrum(ssr.truncated(FULL, 9))
    eng.set_watch(list(range(n)))
    rows, final = _launches(eng, st, pv, n, [7], True)
    a, b = stx.samples_of(rows, None, 0), stx.samples_of(rows, None, 5)
    lev = sc.gap_levels(np.stack([a[0], b[0]], axis=1), n)
    record = _record(eng, n)
    again, state = _launches(eng, st, pv, n, [7], True, record=record, levels=lev, channels=(0, 5))
    vc.assert_same_bits(again, rows, n)
    vc.assert_same_bits(state, final, n)
    got = _host(record, n)
    sc.check_record(got, a, b, lev, None, n)
    assert (got["n"] == 7).all() and np.isfinite(got["sums"]).mean() >= 0.98 and _padding_is_nan(record, n)
    assert (n % 64 == 0) == (not (~live_words(n, 704)).any())       # (64 and 256: no padding lane at all)
    eng.close()


# ---- 5. isolation of the record -----------------------------------------------------------------------------------------------------------------
@COEFFS
def test_a_poisoned_body_leaves_every_other_record(coeff, pop, engines):  # noqa: F811
    """The poison table in the state, channels (x, z), the regular sea, the bed and the lines, 7 steps, implicit drag: every other
    body's eleven words are those of the clean launch; the clean launch afterwards gives the clean record; the poisoned bodies' own
    words are fold of their own rows, and where a body's last sample is a NaN bit 31 of its word is set."""
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        st, pv = pop["st"][:n], pop["pv"][:n]
        ps, pp, bodies, _ = vc.poison(st, pv, n)
        kw = dict(mooring=_tiled(pop["moor"][:n]))
        rows, _ = _launches(eng, st, pv, n, [7], True, **kw)
        lev = sc.gap_levels(np.stack([rows[0][:, 0], rows[0][:, 2]], axis=1), 5 * n)

        def run(s, p):
            record = _record(eng, n)
            r, _ = _launches(eng, s, p, n, [7], True, record=record, levels=lev, channels=(0, 2), **kw)
            return r, _host(record, n)
        (_, want), (bad_rows, got), (_, again) = run(st, pv), run(ps, pp), run(st, pv)
        others = ~np.isin(np.arange(n), bodies)
        assert not sc.body_differs({k: v[others] for k, v in got.items()}, {k: v[others] for k, v in want.items()}).any(), n
        assert sc.same_record(again, want) and sc.same_record(want, stx.fold(None, rows[:, :, 0], rows[:, :, 2], lev))
        sc.check_record(got, bad_rows[:, :, 0], bad_rows[:, :, 2], lev, None, (n, "the poisoned bodies' own words"))
        nan_last = np.stack([np.isnan(bad_rows[-1][:, 0]), np.isnan(bad_rows[-1][:, 2])], axis=1)
        assert nan_last[bodies].any() and not nan_last[others].any() and (got["up"][nan_last] >> 31).all()
        assert np.isnan(got["sums"][bodies]).any() and sc.body_differs(got, want)[bodies].any()
