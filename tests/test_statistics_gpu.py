"""Response statistics on the device (hydro_statistics_reset, hydro_step_fused_tiled_multi_stat): every word of the record is,
bit for bit, `statistics.fold` - the header's arithmetic in NumPy float64 - over the samples the launch took: the recorder's rows
for the motion and velocity channels, the tensions of seven one-step launches for the tension channel; the record accumulates
over launches, chunks and graph replays, `n` included; up-crossings really occur; nothing feeds back - everything else a launch
writes is the _irr entry's bits, with and without every option, in still water, in a regular sea and in spectra of 11 and 64
components; guard bands, padding lanes and refusals; ClosedLoopSim's runners; the example.

Sizes: n = 65 (one live lane in the second tile), 200 (one block: three full tiles and 8 lanes) and 321 (two blocks).  The
population and the mooring records are those of tests/test_mooring_gpu.py; the spread and the net those of
tests/test_mooring_spread_gpu.py.  Every comparison is exact: the policy's arithmetic is IEEE double, one rounding per
operation, and no tolerance is needed or given."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sea_spectrum_reference as ssr
import statistics_reference as sx
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.extremes import Extremes
from silver2_isaacsim_amd.mooring import MooringSpread
from silver2_isaacsim_amd.sea import jonswap, SeaSpectrum, SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population, moored_pop  # noqa: F401  (fixtures are requested by name)
from mooring_spread_population import spread_population
from resident_harness import (_buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, _from, _guarded, _in_one_allocation, _ke, _log, NAN, _rows, S_A, S_C, S_IN, S_OUT, S_PV,
                              S_PVO, _same_bits, _tiled, _unguard, _untouched, _watched)
from tether_net_population import net_for, net_population

pytestmark = pytest.mark.gpu
SIZES = (65, 200, 321)
STEPS = (1, 7)
FULL = ssr.designed_spectrum()                                    # 64 components, U = (0.5, -0.2, 0.05)
CURRENT = SeaState((0.5, -0.2, 0.05))                             # a sea a captured launch can replay: no waves
S_E, S_T2, S_P2, S_SP3 = 8 * 64 + 36, 448 * 2 + 44, 64 * 2 + 20, 576 * 3 + 52      # extremes, a two-layer net, its link tensions, a spread of three
STRIDES = (S_IN, S_PV, S_OUT, S_PVO)
# each of X .. VZ in slot a and in slot b
PAIRS = ((0, 3), (1, 4), (2, 5), (3, 0), (4, 1), (5, 2))


@pytest.fixture(scope="module")
def pop(bed_pop):
    """tests/test_mooring_spread_gpu.py's population: 321 bodies over the bed with the designed spread and the tether net."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, _ = net_population()
    st, pv = st[:321], pv[:321]
    spread = spread_population(st, params["f32"], line_population(st, params["f32"]))
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, spread=spread, net=net)


def _record(eng, n):
    """A fresh record: NaN everywhere, then reset - so the reset has written every live word."""
    return eng.statistics_reset(torch.full((eng.tiles(n), nat.STAT_FIELDS, 64), NAN, dtype=torch.float32, device=DEV), n)


def _host(record, n):
    return stx.unpack(record.cpu().numpy(), n)


def _levels_for(st, n, pair, seed):
    """(n, 2) fp32 levels near the initial values of the two channels: some above, some below, some equal."""
    rng = np.random.default_rng(seed)
    lev = np.stack([st[:n, stx.STATE_FIELD[c]] for c in pair], axis=1).astype(np.float32)
    return (lev + rng.choice(np.array([-1e-3, 0.0, 1e-3], np.float32), size=lev.shape)).astype(np.float32)


# ---- 1. motion and velocity channels: the fold of the recorded rows -----------------------------------------------------------------------
@COEFFS
@DRAG
def test_motion_and_velocity_channels_are_the_fold_of_the_recorded_rows(coeff, implicit, moored_pop, native_built):
    """Every word of the record after a launch of 1 and of 7 steps, with sea, bed, a line, applied wrench and pose hold acting and
    every body recorded: statistics.fold over the recorder's rows of the same launch, for each of X .. VZ in slot a and in slot b."""
    st, pv, params, applied, ctl, rec = moored_pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        lines, a, c17 = _tiled(rec[:n]), _tiled(applied[:n]), _tiled(ctl[:n])
        for steps in STEPS:
            for i, pair in enumerate(PAIRS):
                lev = _levels_for(st, n, pair, 100 * n + i)
                cur, old = _buffers(st, pv, n)
                record, log = _record(eng, n), _log(steps, n)
                torch.cuda.synchronize()
                assert sx.same_record(_host(record, n), stx.empty(n), nan_equal=False)
                sx.launch(eng, cur, old, n, DT, steps, step0=3, statistics=record, levels=_tiled(lev), channels=pair, spread=lines, layers=1,
                          control=c17, applied=a, implicit=implicit, log=log)
                torch.cuda.synchronize()
                rows = _rows(log)[:, :, :13]
                want = stx.fold(None, stx.samples_of(rows, None, pair[0]), stx.samples_of(rows, None, pair[1]), lev)
                got = _host(record, n)
                assert sx.same_record(got, want), (n, steps, pair)
                assert (got["n"] == steps).all()
        eng.close()


# ---- 2. the tension channel ------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_tension_over_seven_single_steps_is_the_fold_of_the_seven_tensions(coeff, implicit, moored_pop, native_built):
    """Seven one-step launches, each with an extremes record reset to empty, so that tension_max of each is that step's T; the
    statistics accumulate over the seven: fold over those seven T's, bit for bit - in slot a against a level of 50 N, in slot b
    against +0, where the count is the number of slack-to-taut events.  A body without a taut line: sums +0, count 0."""
    st, pv, params, _, _, rec = moored_pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines = _tiled(rec[:n])
        lev = np.tile(np.array([50.0, 0.0], np.float32), (n, 1))
        levels = _tiled(lev)
        cur, old = _buffers(st, pv, n)
        record = _record(eng, n)
        T = np.zeros((7, n), np.float32)
        finite = np.isfinite(st[:n]).all(axis=1)
        for k in range(7):
            one = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            sx.launch(eng, cur, old, n, DT, 1, step0=100 + k, statistics=record, levels=levels, channels=(6, 6), spread=lines, layers=1, extremes=one,
                      implicit=implicit)
            cur, old = old, cur
            torch.cuda.synchronize()
            T[k] = _from(one, n)[:, 7]
            finite &= np.isfinite(_from(cur, n)).all(axis=1)
        # (tension_max cannot show a NaN tension, and without a pose hold the explicit form carries most of this population out of
        # the fp32 range within seven steps - the fp64 closed loop does the same: 23 % of the first 65 bodies are finite after the
        # seventh - so the sums are compared for the bodies that stay finite: nearly all of them under implicit drag)
        assert finite.mean() >= 0.98 if implicit else finite.any(), n
        got, want = _host(record, n), stx.fold(None, T, T, lev)
        assert (got["n"] == 7).all()
        got, want, T = {k: v[finite] for k, v in got.items()}, {k: v[finite] for k, v in want.items()}, T[:, finite]
        assert sx.same_record(got, want, nan_equal=False), n
        pulled = (T > 0).any(axis=0)
        assert (pulled.mean() >= 0.25 and (~pulled).any()) if implicit else pulled.any(), n
        idle = got["sums"][~pulled]
        assert not idle[:, 2:4].any() and not np.signbit(idle[:, 2:4]).any() and not stx.upcrossings(got, 1)[~pulled].any(), n
        assert (stx.upcrossings(got, 1)[pulled & (T[0] == 0)] >= 1).all()                            # slack in the first step, taut later: one event at least
        eng.close()


# ---- 3. accumulation -------------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, moored_pop, native_built):
    st, pv, params, _, _, rec = moored_pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines = _tiled(rec[:n])
        lev = _levels_for(st, n, (2, 5), n)
        lev[:, 1] = 0.0
        levels = _tiled(lev)

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            record = _record(eng, n)
            done = 0
            for k in chunks:
                sx.launch(eng, cur, old, n, DT, k, step0=100 + done, statistics=record, levels=levels, channels=(2, 6), spread=lines, implicit=implicit)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, _host(record, n)
        (s7, r7), (s1, r1), (s25, r25) = run([7]), run([1] * 7), run([2, 5])
        assert _same_bits(s7, s1) and _same_bits(s7, s25), n
        assert sx.same_record(r7, r1) and sx.same_record(r7, r25), n
        assert (r7["n"] == 7).all() and np.nan_to_num(r7["sums"]).any()
        eng.close()


def test_a_graph_replayed_three_times_equals_three_eager_launches(moored_pop, native_built):
    """Two launches of 3 steps captured (the ping-pong returns to its buffers), replayed three times, against the same six
    launches made eagerly: state and record, n = 18 per body.  A current-only sea, the bed and the lines ride along."""
    st, pv, params, _, _, rec = moored_pop
    n = 321
    eng = _engine(n, params["f32"], "f32")
    eng.set_sea(CURRENT)
    eng.set_seabed(BED)
    lines = _tiled(rec[:n])
    lev = _levels_for(st, n, (2, 5), 7)
    lev[:, 1] = 0.0
    levels = _tiled(lev)
    stream = torch.cuda.Stream(DEV)

    def pair(cur, old, record):
        kw = dict(statistics=record, levels=levels, channels=(2, 6), spread=lines, implicit=True, stream=stream)
        sx.launch(eng, cur, old, n, DT, 3, **kw)
        sx.launch(eng, old, cur, n, DT, 3, **kw)
    cur, old = _buffers(st, pv, n)
    record = _record(eng, n)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            pair(cur, old, record)
    stream.synchronize()
    want_state, want = cur.clone(), _host(record, n)
    cur, old = _buffers(st, pv, n)
    record = _record(eng, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            pair(cur, old, record)
        torch.cuda.synchronize()
        assert sx.same_record(_host(record, n), stx.empty(n))     # capturing records, it does not execute
        for _ in range(3):
            g.replay()
    stream.synchronize()
    assert _same_bits(cur, want_state) and sx.same_record(_host(record, n), want)
    assert (want["n"] == 18).all()
    eng.close()


# ---- 4. up-crossings really occur --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_upcrossings_in_a_wave_of_a_few_steps(n, native_built):
    """Config 1's buoys in a regular wave whose period is six steps, 24 steps in one launch, channels (vz, z).  The fp64 closed loop
    alone shows what to expect: about its mean every body's vz crosses upwards three or four times.  On the device the levels are
    the means of a first, recorded run of the same launch; the EXPECTED counts - fold over those rows - must be non-zero for at
    least a quarter of the bodies and >= 2 for at least one, and the record of a second run equals the fold bit for bit."""
    _, _, ref = sx.crossing_reference(n)
    ref_up = stx.upcrossings(ref, 0)
    assert (ref_up > 0).mean() >= 0.25 and (ref_up >= 2).any()
    st, pv, pr, sc, dt, sea = sx.crossing_scene(n)
    eng = _engine(n, pr, "f32")
    eng.set_scene(sc.rho, sc.g)
    eng.set_sea(sea)
    eng.set_watch(list(range(n)))
    cur, old = _buffers(st, pv, n)
    log = _log(sx.CROSS_STEPS, n)
    eng.step_fused_tiled_multi_irr(cur, old, n, dt, sx.CROSS_STEPS, 0, implicit_drag=True, log=log)
    torch.cuda.synchronize()
    rows = _rows(log)[:, :, :13]
    lev = sx.levels_of(rows)
    want = stx.fold(None, rows[:, :, 9], rows[:, :, 2], lev)
    expected = stx.upcrossings(want, 0)
    assert (expected > 0).mean() >= 0.25 and (expected >= 2).any(), expected
    cur, old = _buffers(st, pv, n)
    record = _record(eng, n)
    sx.launch(eng, cur, old, n, dt, sx.CROSS_STEPS, statistics=record, levels=_tiled(lev), channels=(5, 2), implicit=True)
    torch.cuda.synchronize()
    got = _host(record, n)
    assert sx.same_record(got, want, nan_equal=False)
    assert np.array_equal(stx.upcrossings(got, 0), expected)
    eng.close()


# ---- 5. the ladder row: nothing feeds back ---------------------------------------------------------------------------------------------------
def _irr(eng, cur, old, n, steps, *, step0=0, spread=None, layers=1, tether=None, net_layers=1, peaks=None, extremes=None, applied=None, frame="world",
         control=None, implicit=False, ke=None, **kw):
    eng.step_fused_tiled_multi_irr(cur, old, n, DT, steps, step0, spread, layers, tether, net_layers, peaks, extremes, control, applied, frame,
                                   implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def _everything(eng, which, pop, n, steps, step0, implicit, ke=None, bare=False, **kw):
    """A launch of the _irr entry ("irr"), of the _stat entry without a record ("null") or with one ("stat"), with the spread of three,
    the two-layer net with its link tensions, extremes, pose hold, applied wrench and a log - or, bare, with nothing.  Returns
    (everything the _irr entry writes, the statistics record or None)."""
    cur, old = _buffers(pop["st"], pop["pv"], n)
    record = _record(eng, n) if which == "stat" else None
    if which != "irr":
        lev = _levels_for(pop["st"], n, (2, 5), n)
        lev[:, 1] = 0.0
        kw.update(statistics=record, levels=_tiled(lev) if which == "stat" else None, channels=(2, 6))
    go = (lambda *a, **k: _irr(eng, *a, **k)) if which == "irr" else (lambda cur, old, n, steps, **k: sx.launch(eng, cur, old, n, DT, steps, **k))
    if bare:
        state, prev = go(cur, old, n, steps, step0=step0, implicit=implicit, ke=ke, **kw)
        torch.cuda.synchronize()
        return [state, prev] + ([ke] if ke is not None else []), record
    watched = _watched(n, (0, 63, 64))
    eng.set_watch(watched)
    log = torch.full((steps, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
    extremes, peaks = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
    state, prev = go(cur, old, n, steps, step0=step0, spread=_tiled(pop["spread"][:n, 0:27]), layers=3, tether=_tiled(net_for(pop["net"], n, 2)),
                     net_layers=2, peaks=peaks, extremes=extremes, applied=_tiled(pop["applied"][:n]), control=_tiled(pop["ctl"][:n]), frame="body",
                     implicit=implicit, ke=ke, log=log, **kw)
    torch.cuda.synchronize()
    return [state, prev, log, extremes, peaks] + ([ke] if ke is not None else []), record


def _same_or_nan(a, b):
    i = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(((a.contiguous().view(i) == b.contiguous().view(i)) | (torch.isnan(a) & torch.isnan(b))).all())


SEAS = {"still": None, "sea": SEA, "irr11": ssr.truncated(FULL, 11), "irr64": FULL}


def _set_water(eng, water):
    eng.set_sea(None)
    eng.set_sea_spectrum(None)
    if isinstance(water, SeaSpectrum):
        eng.set_sea_spectrum(water)
    elif water is not None:
        eng.set_sea(water)


@COEFFS
@DRAG
@pytest.mark.parametrize("water", list(SEAS))
def test_null_is_the_irr_entry_and_a_record_changes_no_other_bit(water, coeff, implicit, pop, native_built):
    """statistics == NULL: the _irr entry's launch.  With a record: state_out, prev_out, the energy pair, the log, the extremes
    and the link tensions are the _irr entry's - everything on, and nothing - and the record has counted the steps."""
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_seabed(BED)
        _set_water(eng, SEAS[water])
        for bare in (False, True):
            want, _ = _everything(eng, "irr", pop, n, 7, 5, implicit, ke=_ke(), bare=bare)
            null, _ = _everything(eng, "null", pop, n, 7, 5, implicit, ke=_ke(), bare=bare)
            got, record = _everything(eng, "stat", pop, n, 7, 5, implicit, ke=_ke(), bare=bare)
            assert len(null) == len(want) and all(_same_or_nan(x, y) for x, y in zip(null, want)), (n, bare)
            assert len(got) == len(want) and all(_same_or_nan(x, y) for x, y in zip(got, want)), (n, bare)
            rec = _host(record, n)
            assert (rec["n"] == 7).all() and np.nan_to_num(rec["sums"][:, 0:2]).any()
        eng.close()


def test_every_option_on_its_own(pop, native_built):
    """n = 65, 2 steps, f32, explicit, with the kinetic energy, in still water: each option alone - and none - with a record."""
    n, steps, step0 = 65, 2, 3
    st, pv = pop["st"], pop["pv"]
    lev = _levels_for(st, n, (0, 4), 3)
    for option in (None, "log", "applied", "control", "sea", "seabed", "spread", "extremes", "net", "peaks"):
        eng = _engine(n, pop["params"]["f32"], "f32")
        eng.set_watch([0, 5, 63, 64])
        eng.set_sea(SEA if option == "sea" else None)
        eng.set_seabed(BED if option == "seabed" else None)
        layers = 2 if option in ("net", "peaks") else 1

        def run(with_record):
            cur, old = _buffers(st, pv, n)
            ke = _ke()
            log = torch.full((steps, 19, 4), NAN, dtype=torch.float32, device=DEV) if option == "log" else None
            extremes = eng.extremes_reset(eng.alloc_tiled(8, n), n) if option == "extremes" else None
            peaks = eng.alloc_tiled(layers, n) if option == "peaks" else None
            kw = dict(step0=step0, spread=_tiled(pop["spread"][:n, 0:27]) if option == "spread" else None, layers=3,
                      tether=_tiled(net_for(pop["net"], n, layers)) if option in ("net", "peaks") else None, net_layers=layers, peaks=peaks,
                      extremes=extremes, applied=_tiled(pop["applied"][:n]) if option == "applied" else None,
                      control=_tiled(pop["ctl"][:n]) if option == "control" else None, frame="body", ke=ke, log=log)
            record = _record(eng, n) if with_record else None
            if with_record:
                state, prev = sx.launch(eng, cur, old, n, DT, steps, statistics=record, levels=_tiled(lev), channels=(0, 4), **kw)
            else:
                state, prev = _irr(eng, cur, old, n, steps, **kw)
            torch.cuda.synchronize()
            return [state, prev, ke] + [x for x in (log, extremes, peaks) if x is not None], record
        (want, _), (got, record) = run(False), run(True)
        assert len(got) == len(want) and all(_same_bits(x, y) for x, y in zip(got, want)), option
        assert (_host(record, n)["n"] == steps).all(), option
        eng.close()


@COEFFS_SEMANTICS
@pytest.mark.parametrize("water", ["sea", "irr64"])
def test_energy_and_non_temporal_instantiations(water, coeff, semantics, pop, native_built):
    """KE = true and NT = true (set_tuning(0, 0, 1)) in both semantics, with everything on, for both kernel families: the record
    and every other output are those of the launch without sampling and of the temporal launch."""
    n = 321
    eng = _engine(n, pop["params"][coeff], coeff, semantics)
    eng.set_seabed(BED)
    _set_water(eng, SEAS[water])
    eng.set_tuning(0, 0, 0)
    want, want_rec = _everything(eng, "stat", pop, n, 7, 5, True)
    irr, _ = _everything(eng, "irr", pop, n, 7, 5, True)
    assert all(_same_bits(x, y) for x, y in zip(want, irr))
    got, rec = _everything(eng, "stat", pop, n, 7, 5, True, ke=_ke())
    assert all(_same_bits(x, y) for x, y in zip(got, want)) and sx.same_record(_host(rec, n), _host(want_rec, n))
    eng.set_tuning(0, 0, 1)
    for ke in (None, _ke()):
        streamed, srec = _everything(eng, "stat", pop, n, 7, 5, True, ke=ke)
        assert all(_same_bits(x, y) for x, y in zip(streamed, want)) and sx.same_record(_host(srec, n), _host(want_rec, n))
    eng.close()


# ---- 6. guard bands round both records and the padding lanes ------------------------------------------------------------------------------------
def _guarded_record(n):
    return torch.full((((n + 63) // 64) * sx.S_ST,), NAN, dtype=torch.float32, device=DEV)


def _raw_reset(eng, n, buf, stride=sx.S_ST, stream=None):
    p = buf.data_ptr() if hasattr(buf, "data_ptr") else buf
    return eng._lib.hydro_statistics_reset(eng._h, n, p, stride, eng._stream(stream))


def _words(buf):
    return buf.cpu().numpy().view(np.uint32)


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 65 and 200 with tile strides larger than the records and different for every buffer, NaN in the stride padding and in
    the padding lanes: the reset and the step write the live lanes' words and nothing else, the levels' sentinels are neither read
    nor written, and the record is that of the tightly packed launch."""
    st, pv = pop["st"], pop["pv"]
    for n in (65, 200):
        tiles = (n + 63) // 64
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea_spectrum(FULL)
        eng.set_seabed(BED)
        lev = _levels_for(st, n, (2, 5), n)
        lev[:, 1] = 0.0
        state, prev, m27, lv = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["spread"][:n, 0:27], S_SP3), _guarded(lev, sx.S_LV)
        before = [b.cpu().numpy() for b in (state, prev, m27, lv)]
        record = _guarded_record(n)
        assert _raw_reset(eng, n, record) == 0
        torch.cuda.synchronize()
        rec0, rest0 = sx.unguard(_words(record), n)
        assert sx.same_record(rec0, stx.empty(n), nan_equal=False) and (rest0 == sx.NAN_BITS).all()
        out = torch.full((tiles * S_OUT,), NAN, device=DEV)
        pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
        rc, written = sx.raw_stat(eng, n, DT, state, prev, out, pvo, STRIDES, steps=3, step0=11, implicit=implicit, mooring=m27, s_mooring=S_SP3, layers=3,
                                  statistics=record, levels=lv, channels=(2, 6))
        eng._check(rc)
        torch.cuda.synchronize()
        assert written == 0
        got, rest = sx.unguard(_words(record), n)
        state3, srest = _unguard(out, n, 13, S_OUT)
        assert (rest == sx.NAN_BITS).all() and np.isnan(srest).all(), "a sentinel of an output was overwritten"
        assert all(_untouched(b, was) for b, was in zip((state, prev, m27, lv), before))
        cur, old = _buffers(st, pv, n)
        packed = _record(eng, n)
        want_state, _ = sx.launch(eng, cur, old, n, DT, 3, step0=11, statistics=packed, levels=_tiled(lev), channels=(2, 6), spread=_tiled(pop["spread"][:n, 0:27]),
                                  layers=3, implicit=implicit)
        torch.cuda.synchronize()
        assert sx.same_record(got, _host(packed, n)) and (got["n"] == 3).all()
        assert np.array_equal(state3.view(np.uint32), _from(want_state, n).view(np.uint32))
        assert np.isfinite(got["sums"]).all() or not implicit, "a sentinel was read"
        # the tightly packed record's padding lanes: NaN from _record, never written
        assert (_words(packed).reshape(tiles, -1)[~sx.live_words(n, 704)] == sx.NAN_BITS).all()
        eng.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_both_records(pop, native_built):
    n = 321
    tiles = (n + 63) // 64
    eng = _engine(n, pop["params"]["f32"], "f32")
    eng.set_sea_spectrum(FULL)
    st, pv = pop["st"], pop["pv"]
    lev = _levels_for(st, n, (2, 5), 1)
    state, prev, lv = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(lev, sx.S_LV)
    a, c17 = _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m27, net = _guarded(pop["spread"][:n, 0:27], S_SP3), _guarded(net_for(pop["net"], n, 2), S_T2)
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    p2 = torch.full((tiles * S_P2,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    record = _guarded_record(n)
    # one allocation, a fixed order, gaps wider than any record's extent: a buffer handed over as ANOTHER record below makes the
    # library claim that record's extent from its address, and the claim must meet nothing but the buffer itself
    state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record = _in_one_allocation(state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record)
    E_ARG = -1
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    # the reset's own refusals
    assert _raw_reset(eng, n + 1, record) == E_ARG and _raw_reset(eng, n, None) == E_ARG
    assert _raw_reset(eng, n, record.data_ptr() + 8) == E_ARG and _raw_reset(eng, n, record, 700) == E_ARG
    torch.cuda.synchronize()
    assert (_words(record) == sx.NAN_BITS).all()
    assert _raw_reset(eng, n, record) == 0
    torch.cuda.synchronize()
    was, lv_was = _words(record).copy(), lv.cpu().numpy()
    everything = dict(applied=a, s_applied=S_A, control=c17, s_control=S_C, mooring=m27, s_mooring=S_SP3, layers=3, extremes=e8, s_extremes=S_E,
                      tether=net, s_tether=S_T2, net_layers=2, peaks=p2, s_peaks=S_P2)

    def call(**kw):
        args = dict(everything, statistics=record, levels=lv)
        args.update(kw)
        return sx.raw_stat(eng, n, DT, state, prev, out, pvo, STRIDES, **args)
    # the _irr entry's refusals come first, with and without a record
    assert call(step0=-1) == (E_ARG, -7) and call(steps=0) == (E_ARG, -7)
    assert call(layers=5) == (E_ARG, -7) and "mooring_layers" in last()
    assert call(statistics=None, levels=None, net_layers=5) == (E_ARG, -7) and "tether_layers" in last()
    # then the channels - also without a record -
    for bad in ((7, 0), (0, 7), (-1, 2), (2, -1)):
        assert call(channels=bad) == (E_ARG, -7) and "channel" in last(), bad
        assert call(channels=bad, statistics=None, levels=None) == (E_ARG, -7) and "channel" in last(), bad
    # a null level record, the two records' own layout
    assert call(levels=None) == (E_ARG, -7) and "levels" in last()
    assert call(statistics=record.data_ptr() + 8) == (E_ARG, -7) and call(s_statistics=700) == (E_ARG, -7)
    assert call(levels=lv.data_ptr() + 4) == (E_ARG, -7) and call(s_levels=124) == (E_ARG, -7)
    # statistics overlapping an output or - it is written - an input; levels overlapping an output
    for name, other in (("state_out", out), ("prev_out", pvo), ("extremes", e8), ("tether_peaks", p2)):
        assert call(statistics=other) == (E_ARG, -7) and "statistics must not overlap an output" in last(), name
    for name, other in (("state", state), ("prev", prev), ("applied", a), ("control", c17), ("mooring", m27), ("tether", net)):
        assert call(statistics=other) == (E_ARG, -7) and "statistics must not overlap an input" in last(), name
    assert call(levels=record.data_ptr() + 16, s_levels=sx.S_ST) == (E_ARG, -7) and "statistics must not overlap an input" in last()
    for name, other in (("state_out", out), ("prev_out", pvo), ("extremes", e8), ("tether_peaks", p2)):
        assert call(levels=other) == (E_ARG, -7) and "levels must not overlap an output" in last(), name
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (out, pvo, e8, p2))
    assert np.array_equal(_words(record), was) and _untouched(lv, lv_was)
    # the legal launch next to them
    e8.copy_(_guarded(Extremes.empty(n), S_E))
    p2.copy_(_guarded(np.zeros((n, 2), np.float32), S_P2))
    assert call(steps=3, extremes=e8, peaks=p2) == (0, 0)
    torch.cuda.synchronize()
    got, rest = sx.unguard(_words(record), n)
    assert (got["n"] == 3).all() and (rest == sx.NAN_BITS).all() and _untouched(lv, lv_was)
    eng.close()


# ---- 8, 9. ClosedLoopSim and the example ---------------------------------------------------------------------------------------------------------
def _moored_sim(sc, sea):
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    mass = float(sc.params[0, 10])
    k0, c0 = MooringSpread.for_body(mass, sc.dt, 3)
    centre = sc.state[:, 0:2].astype(np.float64)
    reach = float(np.hypot(15.0, 20.0 + float(sc.state[0, 2])))
    length, k = np.full((sc.n, 3), reach - 0.2), np.full((sc.n, 3), k0)
    lines = MooringSpread.radial(3, 15.0, 20.0, centre=centre, length=length, stiffness=k, damping=c0)
    sim.set_mooring_spread(lines.anchors, length=length, stiffness=k, damping=c0)
    return sim


def _buoy_field(n=200):
    c1 = scenes.scene_c1()
    pr = np.tile(c1.params[:1].astype(np.float32), (n, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(n)
    st = np.zeros((n, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = 37.0 * (i % 16), 41.0 * (i // 16), z_eq, 1.0
    return scenes.Scene("statistics", st, np.zeros((n, 6), np.float32), pr, dt=float(np.float32(1.0 / 60.0)), rho=c1.rho, g=c1.g)


def test_sim_track_statistics_resident_equals_eager_and_clear_statistics(native_built):
    sc = _buoy_field()
    sea = jonswap(1.5, 7.0, 25.0, spread="cos2", seed=3, current=(0.4, 0.0, 0.0), g=sc.g)
    records, finals, extremes = {}, {}, {}
    for name, go in (("eager", lambda s: s.run_eager(20)), ("resident", lambda s: s.run_resident(20)), ("chunks", lambda s: s.run_resident(20, chunk=7))):
        sim = _moored_sim(sc, sea)
        ext = sim.track_extremes()
        stat = sim.track_statistics()
        assert stat is sim.statistics and stat.channels == ("z", "tension") and not stat.levels[:, 1].any()
        assert np.array_equal(stat.levels[:, 0], sc.state[:, 2])
        go(sim)
        records[name], finals[name], extremes[name] = stat.record(), sim.state(), ext.bodies()
        if name == "resident":
            assert (stat.count() == 20).all() and np.isfinite(stat.std("z")).all() and (stat.mean("tension") >= 0).all()
            mpm = stat.most_probable_maximum("tension", steps=3600)
            assert np.isfinite(mpm).all() and (mpm >= stat.mean("tension")).all()
            with pytest.raises(ValueError, match="reset"):
                sim.track_statistics(("x", "tension"))
            again = sim.track_statistics(("x", "tension"), reset=True)
            assert again is stat and again.buffer.data_ptr() == stat.buffer.data_ptr() and (again.count() == 0).all()
            sim.clear_statistics()
            assert sim.statistics is None
            sim.run_resident(5)
            assert (again.count() == 0).all()                     # no longer tracked: the record keeps its contents
        sim.close()
    for k in ("resident", "chunks"):
        assert sx.same_record(records["eager"], records[k], nan_equal=False), k
        assert np.array_equal(finals["eager"], finals[k]) and np.array_equal(extremes["eager"], extremes[k])
    plain = _moored_sim(sc, sea)
    plain.track_extremes()
    plain.run_resident(20)
    assert np.array_equal(plain.state(), finals["eager"]) and np.array_equal(plain.extremes.bodies(), extremes["eager"])     # nothing feeds back
    plain.close()
    # graph replays: a current-only sea rides, and equals the resident run; lines + waves stay refused
    g, r = _moored_sim(sc, SeaState((0.4, -0.1, 0.0))), _moored_sim(sc, SeaState((0.4, -0.1, 0.0)))
    gs, rs = g.track_statistics(("x", "tension")), r.track_statistics(("x", "tension"))
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and sx.same_record(gs.record(), rs.record(), nan_equal=False) and (gs.count() == 64).all()
    waves = _moored_sim(sc, sea)
    waves.track_statistics()
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    for s in (g, r, waves):
        s.close()


def test_mooring_response_statistics_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "mooring_response_statistics.py"), "--steps", "240"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    assert len(re.findall(r"most probable maximum +([\d.]+) N", res.stdout)) == 9
    assert "spread of tension_max over" in res.stdout
