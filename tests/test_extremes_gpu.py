"""Per-body extremes on the device (hydro_extremes_reset, hydro_step_fused_tiled_multi_ext): the position fields and
speed2_max are, bit for bit, Extremes.fold over the rows the recorder wrote in the same launch; tension_max follows
mooring_reference.tension after one step and is the maximum of seven one-step launches after seven; the record accumulates
over launches, chunks and graph replays; nothing feeds back - states, energy and log are the mooring entry's bits with and
without every option; guard bands, padding lanes and refusals; ClosedLoopSim's runners; the example.

Sizes: n = 200 (one block: three full tiles and 8 lanes) and n = 321 (two blocks, the last wave with one live lane).  The
population and the mooring records are those of tests/test_mooring_gpu.py.  Every body is on the watch list and every step
is recorded with its wrench.

THE TENSION BOUND.  Errors of tension_max after one step against mooring_reference.tension (fp64), in units of 2^-24 of
extremes_reference.tension_scale = k (l^ + L0) + c u^, over the designed population, the eight bodies at the tie aside.  The
rule: the next power of two at or above twice the largest.  TENSION_BOUND = 2 stands on the header's fp32 order emulated on
the host over this population (tests/test_extremes.py): 0.77; 2 x 0.77 = 1.53.  On an MI355X: 0.77, f32 and f16
coefficients alike; the bound stays 2.  The test prints the device's figure.

speed2_max is compared exactly: extremes.fma32 rounds once (tests/test_extremes.py holds it to rational arithmetic), so the
host's chain is the kernel's, with or without math.fma."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import extremes_reference as er
import mooring_reference as mr
from conftest import REPO
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd.extremes import Extremes
from silver2_isaacsim_amd.mooring import Mooring
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop, SEA, SIZES, STEPS  # noqa: F401  (fixtures are requested by name)
from mooring_population import _buoys, DEPTH, moored_pop as pop, OFF_TIES, TIES  # noqa: F401  (fixtures are requested by name)
from resident_harness import (_buffers, COEFFS, DEV, DRAG, _engine, _from, _guarded, _ke, _log, NAN, raw, _rows, S_A, S_C, S_IN, S_M, S_OUT, S_PV, S_PVO,
                              _same_bits, step, _tiled, _unguard, _untouched)

pytestmark = pytest.mark.gpu
S_E = 8 * 64 + 44                                                 # the extremes record's tile stride in the guard tests
CURRENT = SeaState((0.5, -0.2, 0.05))                             # a sea a captured launch can replay: no waves


def _record(eng, n, state=None):
    """A fresh record: reset, or seeded from the tiled `state`."""
    return eng.extremes_reset(torch.full((eng.tiles(n), 8, 64), NAN, dtype=torch.float32, device=DEV), n, state)


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1, 2. positions and speed2: the fold of the recorded rows -------------------------------------------------------------------------
@COEFFS
@DRAG
def test_positions_and_speed2_are_the_fold_of_the_recorded_rows(coeff, implicit, pop, native_built):
    """Fields 0 .. 6 after a launch of 1 and of 7 steps, from a reset and from a state-seeded record, with sea, bed, lines,
    applied wrench and pose hold acting: Extremes.fold over the recorder's rows of the same launch, bit for bit."""
    st, pv, params, applied, ctl, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        lines, a, c17 = _tiled(rec[:n]), _tiled(applied[:n]), _tiled(ctl[:n])
        for steps in STEPS:
            for seeded in (False, True):
                cur, old = _buffers(st, pv, n)
                record, log = _record(eng, n, cur if seeded else None), _log(steps, n)
                torch.cuda.synchronize()
                seed = _from(record, n)
                assert _eq(seed, ex.seed_of(st[:n]) if seeded else Extremes.empty(n)), (n, seeded)
                step(eng, "ext", cur, old, n, steps, step0=3, extremes=record, mooring=lines, control=c17, applied=a, implicit=implicit, log=log)
                torch.cuda.synchronize()
                got, rows = _from(record, n), _rows(log)
                want = Extremes.fold(rows[:, :, :13], np.zeros((steps, n), np.float32), seed)
                assert not np.isnan(got).any()
                assert _eq(got[:, 0:6], want[:, 0:6]), (n, steps, seeded)
                assert _eq(got[:, 6], want[:, 6]), (n, steps, seeded, np.abs(got[:, 6] - want[:, 6]).max())
                assert (got[:, 1] >= got[:, 0]).all() and (got[:, 6] >= 0).all()
        eng.close()


# ---- 3. the tension --------------------------------------------------------------------------------------------------------------------
@COEFFS
def test_tension_after_one_step_against_the_reference(coeff, pop, native_built):
    st, pv, params, _, _, rec = pop
    worst = 0.0
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        s, m, off = st[:n], rec[:n], OFF_TIES[:n]
        for lines in (_tiled(m), None):
            cur, old = _buffers(st, pv, n)
            record = _record(eng, n)
            step(eng, "ext", cur, old, n, 1, extremes=record, mooring=lines)
            torch.cuda.synchronize()
            got = _from(record, n)[:, ex.TENSION_MAX]
            if lines is None:                                    # no mooring record at all: exactly +0 for everybody
                assert not got.any() and not np.signbit(got).any(), n
                continue
            ref, scale = mr.tension(m, s), er.tension_scale(m, s)
            live = (ref > 0) & off
            idle = ~live & off
            assert live.mean() >= 0.25 and (got[live] > 0).all(), (n, live.mean())               # at least a quarter pull, by the reference
            assert not got[idle].any() and not np.signbit(got[idle]).any(), n                    # not taut (or clamped, or no line): +0
            err = np.abs(got[live].astype(np.float64) - ref[live]) / (mr.ULP * scale[live])
            worst = max(worst, float(err.max()))
            # the ties: l within 2 ulps of L0 - the taut value or nothing (without a damper the taut value is itself next to nothing)
            everyone = np.ones(n, bool)
            taut_ref = mr.tension(m, s, everyone)
            for b in TIES:
                assert got[b] == 0 or abs(float(got[b]) - taut_ref[b]) <= er.TENSION_BOUND * mr.ULP * scale[b], (b, got[b], taut_ref[b])
        eng.close()
    print(f"[extremes, tension_max after one step, {coeff}] largest error {worst:.3f} units of 2^-24 of the scale (bound {er.TENSION_BOUND:g})")
    assert worst <= er.TENSION_BOUND


@COEFFS
@DRAG
def test_tension_after_seven_steps_is_the_maximum_of_seven_single_steps(coeff, implicit, pop, native_built):
    """tension_max of one launch of 7 steps = the compare-and-select maximum over seven launches of one step, each from a
    reset record, bit for bit; so are the other seven fields (their fold)."""
    st, pv, params, _, _, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines = _tiled(rec[:n])
        cur, old = _buffers(st, pv, n)
        whole = _record(eng, n)
        step(eng, "ext", cur, old, n, 7, step0=100, extremes=whole, mooring=lines, implicit=implicit)
        cur, old = _buffers(st, pv, n)
        want = Extremes.empty(n)
        pulled = np.zeros(n, bool)
        for k in range(7):
            one = _record(eng, n)
            step(eng, "ext", cur, old, n, 1, step0=100 + k, extremes=one, mooring=lines, implicit=implicit)
            cur, old = old, cur
            torch.cuda.synchronize()
            r = _from(one, n)
            pulled |= r[:, 7] > 0
            for f in range(8):
                x, acc = r[:, f], want[:, f]
                want[:, f] = np.where(x < acc, x, acc) if f in (0, 2, 4) else np.where(x > acc, x, acc)
        torch.cuda.synchronize()
        assert _eq(_from(whole, n), want), n
        assert pulled.mean() >= 0.25
        eng.close()


# ---- 4. accumulation ---------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks_and_a_second_launch_only_widens(coeff, implicit, pop, native_built):
    st, pv, params, _, _, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines = _tiled(rec[:n])

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            record = _record(eng, n, cur)
            done, history = 0, []
            for k in chunks:
                step(eng, "ext", cur, old, n, k, step0=100 + done, extremes=record, mooring=lines, implicit=implicit)
                cur, old = old, cur
                done += k
                torch.cuda.synchronize()
                history.append(_from(record, n))
            return cur, history
        (s7, h7), (s1, h1), (s25, h25) = run([7]), run([1] * 7), run([2, 5])
        assert _same_bits(s7, s1) and _same_bits(s7, s25), n
        assert _eq(h7[-1], h1[-1]) and _eq(h7[-1], h25[-1]), n
        for before, after in zip(h1, h1[1:]):                    # a later launch never lowers a max or raises a min
            assert (after[:, [1, 3, 5, 6, 7]] >= before[:, [1, 3, 5, 6, 7]]).all() and (after[:, [0, 2, 4]] <= before[:, [0, 2, 4]]).all(), n
        assert not _eq(h1[0], h1[-1])
        eng.close()


def test_a_graph_replayed_three_times_equals_three_eager_launches(pop, native_built):
    """Two launches of 3 steps captured (the ping-pong returns to its buffers), replayed three times, against the same six
    launches made eagerly: state and record.  A current-only sea, the bed and the lines ride along."""
    st, pv, params, _, _, rec = pop
    n = 321
    eng = _engine(n, params["f32"], "f32")
    eng.set_sea(CURRENT)
    eng.set_seabed(BED)
    lines = _tiled(rec[:n])
    stream = torch.cuda.Stream(DEV)

    def pair(cur, old, record):
        step(eng, "ext", cur, old, n, 3, extremes=record, mooring=lines, implicit=True, stream=stream)
        step(eng, "ext", old, cur, n, 3, extremes=record, mooring=lines, implicit=True, stream=stream)
    cur, old = _buffers(st, pv, n)
    record = _record(eng, n, cur)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            pair(cur, old, record)
    stream.synchronize()
    want_state, want = cur.clone(), _from(record, n)
    cur, old = _buffers(st, pv, n)
    record = _record(eng, n, cur)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            pair(cur, old, record)
        torch.cuda.synchronize()
        assert _eq(_from(record, n), ex.seed_of(st[:n]))         # capturing records, it does not execute
        for _ in range(3):
            g.replay()
    stream.synchronize()
    assert _same_bits(cur, want_state) and _eq(_from(record, n), want)
    assert (want[:, 7] > 0).mean() >= 0.25
    eng.close()


# ---- 5. nothing feeds back -----------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_no_record_is_the_mooring_entry_and_a_record_changes_no_other_bit(coeff, implicit, pop, native_built):
    """extremes = NULL: the launch of hydro_step_fused_tiled_multi_moor.  With a record: state, prev_out, the energy pair and
    the log (state and wrench of every body, every step) are that entry's bits - with and without each of log, applied
    wrench, control, sea, bed and lines."""
    st, pv, params, applied, ctl, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_watch(list(range(n)))
        a, c17, m9 = _tiled(applied[:n]), _tiled(ctl[:n]), _tiled(rec[:n])
        for sea in (None, SEA):
            for bed in (None, BED):
                eng.set_sea(sea)
                eng.set_seabed(bed)
                for steps in STEPS:
                    for app in (None, a):
                        for control in (None, c17):
                            for lines in (None, m9):
                                for with_log in (False, True):
                                    what = (n, steps, app is None, control is None, lines is None, with_log, sea is None, bed is None)
                                    cur, old = _buffers(st, pv, n)
                                    w_ke, w_log = _ke(), _log(steps, n) if with_log else None
                                    want = step(eng, "moor", cur, old, n, steps, step0=3, mooring=lines, control=control, applied=app, implicit=implicit, ke=w_ke,
                                                **dict(log=w_log) if with_log else {})
                                    for record in (None, _record(eng, n)):
                                        c, o = _buffers(st, pv, n)
                                        ke, log = _ke(), _log(steps, n) if with_log else None
                                        got = step(eng, "ext", c, o, n, steps, step0=3, extremes=record, mooring=lines, control=control, applied=app, implicit=implicit,
                                                   ke=ke, **dict(log=log) if with_log else {})
                                        torch.cuda.synchronize()
                                        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _same_bits(ke, w_ke), what
                                        assert not with_log or _same_bits(log, w_log), what
                                        if record is not None and lines is None:
                                            assert not _from(record, n)[:, 7].any(), what
        eng.close()


@COEFFS
@DRAG
def test_energy_and_non_temporal_instantiations(coeff, implicit, pop, native_built):
    """KE = true and NT = true (set_tuning(0, 0, 1)) of the new kernel, everything acting: state and energy bits of the
    mooring entry, and the record of the temporal launch without sampling."""
    st, pv, params, applied, ctl, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines, a, c17 = _tiled(rec[:n]), _tiled(applied[:n]), _tiled(ctl[:n])

        def run(entry, ke=None):
            cur, old = _buffers(st, pv, n)
            record = _record(eng, n, cur) if entry == "ext" else None
            state, prev = step(eng, entry, cur, old, n, 7, step0=5, extremes=record, mooring=lines, control=c17, applied=a, implicit=implicit, ke=ke)
            torch.cuda.synchronize()
            return state, prev, (_from(record, n) if record is not None else None)
        eng.set_tuning(0, 0, 0)
        plain = run("ext")
        w_ke, ke = _ke(), _ke()
        want, got = run("moor", w_ke), run("ext", ke)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _same_bits(ke, w_ke) and _eq(got[2], plain[2]), n
        assert _same_bits(got[0], plain[0])
        eng.set_tuning(0, 0, 1)
        streamed = run("ext")
        ke_nt = _ke()
        streamed_ke = run("ext", ke_nt)
        eng.set_tuning(0, 0, 0)
        for other in (streamed, streamed_ke):
            assert _same_bits(other[0], plain[0]) and _same_bits(other[1], plain[1]) and _eq(other[2], plain[2]), n
        assert _same_bits(ke_nt, w_ke), n
        eng.close()


# ---- 6. guards and refusals through the raw C ABI ---------------------------------------------------------------------------------------


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64, NaN in the stride padding and in the lanes past body n of every buffer:
    the record is that of the tightly packed launch, and no sentinel of it - guard band or padding lane - is read into a
    body's record or overwritten, by the step entry and by hydro_extremes_reset in both its forms."""
    st, pv, params, applied, ctl, rec = pop
    n, tiles = 200, 4
    eng = _engine(n, params[coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    state, prev, a, c17, m9 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C), _guarded(rec[:n], S_M)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9)]
    lib, h, s = eng._lib, eng._h, eng._stream(None)
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    eng._check(lib.hydro_extremes_reset(h, n, None, 0, e8.data_ptr(), S_E, s))
    torch.cuda.synchronize()
    got, rest = _unguard(e8, n, 8, S_E)
    assert _eq(got, Extremes.empty(n)) and np.isnan(rest).all()
    eng._check(lib.hydro_extremes_reset(h, n, state.data_ptr(), S_IN, e8.data_ptr(), S_E, s))
    torch.cuda.synchronize()
    got, rest = _unguard(e8, n, 8, S_E)
    assert _eq(got, ex.seed_of(st[:n])) and np.isnan(rest).all()
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    rc, _ = raw(eng, "ext", n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, applied=a, control=c17, mooring=m9, extremes=e8, s_extremes=S_E)
    eng._check(rc)
    torch.cuda.synchronize()
    got, rest = _unguard(e8, n, 8, S_E)
    assert np.isnan(rest).all(), "a sentinel of the record was overwritten"
    assert not np.isnan(got).any(), "a sentinel was read"
    assert np.isnan(_unguard(out, n, 13, S_OUT)[1]).all() and np.isnan(_unguard(pvo, n, 6, S_PVO)[1]).all()
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9), before))
    cur, old = _buffers(st, pv, n)
    packed = _record(eng, n, cur)
    want_state, _ = step(eng, "ext", cur, old, n, 3, step0=11, extremes=packed, mooring=_tiled(rec[:n]), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert _eq(got, _from(packed, n)) and _eq(_unguard(out, n, 13, S_OUT)[0], _from(want_state, n))
    eng.close()


def test_refusals_launch_nothing_and_leave_the_record(pop, native_built):
    """The refusals are the mooring entry's, in its order, then the extremes': stride, alignment, overlap with each output and
    each input.  The reset's own.  Nothing is launched: record, outputs and inputs keep their bits."""
    st, pv, params, applied, ctl, rec = pop
    n = 321
    eng = _engine(n, params["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a, c17, m9 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C), _guarded(rec[:n], S_M)
    e8 = _guarded(np.arange(n * 8, dtype=np.float32).reshape(n, 8), S_E)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9, e8)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    e, last = e8.data_ptr(), lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    every = dict(applied=a, control=c17, mooring=m9)
    for bed, sea in ((BED, SEA), (None, None)):
        eng.set_watch(None)
        eng.set_seabed(bed)
        eng.set_sea(sea)
        # the mooring entry's refusals, in its order, with a record
        assert raw(eng, "ext", n, state, prev, out, pvo, step0=-1, extremes=e, s_extremes=S_E, **every) == (E_ARG, -7)
        assert raw(eng, "ext", n, state, prev, out, pvo, steps=0, extremes=e, s_extremes=S_E, **every) == (E_ARG, -7)
        assert raw(eng, "ext", n, state, prev, out, pvo, applied=a.data_ptr() + 4, extremes=e, s_extremes=S_E) == (E_ARG, -7)
        assert raw(eng, "ext", n, state, prev, out, pvo, control=c17.data_ptr() + 4, extremes=e, s_extremes=S_E) == (E_ARG, -7)
        assert raw(eng, "ext", n, state, prev, out, pvo, mooring=m9.data_ptr() + 4, extremes=e, s_extremes=S_E) == (E_ARG, -7)
        assert raw(eng, "ext", n, state, prev, out, pvo, log=log, extremes=e, s_extremes=S_E, **every) == (E_STATE, -7)               # a log without a watch list
        # the mooring's come before the extremes'
        assert raw(eng, "ext", n, state, prev, out, pvo, mooring=out, extremes=e + 4, s_extremes=S_E) == (E_ARG, -7) and "mooring must not overlap" in last()
        # the extremes' own
        assert raw(eng, "ext", n, state, prev, out, pvo, extremes=e + 4, s_extremes=S_E, **every) == (E_ARG, -7) and "16-byte aligned" in last()
        assert raw(eng, "ext", n, state, prev, out, pvo, extremes=e, s_extremes=508, **every) == (E_ARG, -7)              # below 8 * 64
        assert raw(eng, "ext", n, state, prev, out, pvo, extremes=e, s_extremes=514, **every) == (E_ARG, -7)              # not a multiple of 4
        for output in (out, pvo):
            assert raw(eng, "ext", n, state, prev, out, pvo, extremes=output, s_extremes=S_E, **every) == (E_ARG, -7) and "extremes must not overlap an output" in last()
        for inp in (state, prev, a, c17, m9):
            assert raw(eng, "ext", n, state, prev, out, pvo, extremes=inp, s_extremes=S_E, **every) == (E_ARG, -7) and "extremes must not overlap an input" in last(), last()
        assert raw(eng, "ext", n, state, prev, out, pvo, extremes=state.data_ptr() + 7 * 64 * 4, s_extremes=S_E) == (E_ARG, -7)       # inside the state: its velocity fields
        eng.set_watch([0, 320])
        assert raw(eng, "ext", n, state, prev, out, pvo, log=log, extremes=log, s_extremes=S_E, **every) == (E_ARG, -7) and "extremes must not overlap an output" in last()
    # the reset
    lib, s, sp = eng._lib, eng._stream(None), state.data_ptr()
    for args in ((n, None, 0, None, S_E), (n, None, 0, e + 4, S_E), (n, None, 0, e, 508), (n, None, 0, e, 514), (n + 1, None, 0, e, S_E),
                 (-1, None, 0, e, S_E), (n, sp + 4, S_IN, e, S_E), (n, sp, 828, e, S_E), (n, sp, S_IN, sp, S_E), (n, sp, S_IN, sp + 12 * 64 * 4, S_E)):
        assert lib.hydro_extremes_reset(eng._h, *args, s) == E_ARG, args
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all()
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9, e8), before))
    bare = type(eng)(n, DEV, 1000.0, 9.81)                        # no parameters yet: the reset needs none
    assert lib.hydro_extremes_reset(bare._h, n, None, 0, e, S_E, bare._stream(None)) == 0
    torch.cuda.synchronize()
    bare.close()
    got, rest = _unguard(e8, n, 8, S_E)
    assert _eq(got, Extremes.empty(n)) and np.isnan(rest).all()
    eng.close()


# ---- 7. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------------
def test_sim_the_buoys_in_a_current_resident_equals_eager_and_clear_extremes(native_built):
    """64 moored buoys at different headings in the 0.5 m/s current: 600 steps under run_resident(chunk=64) and under
    run_eager leave bit-identical records (the lines come taut 2 m downstream, about half way through); the resident run also
    records every step of every buoy: the record is Extremes.fold over those rows and its tension_max the largest tension
    the fp64 restatement finds along them; clear_extremes makes the sim the one that never tracked."""
    sc, anchors, z_eq, mass = _buoys()
    k, c = Mooring.for_body(mass, sc.dt)
    L0 = DEPTH + 0.1
    lines = Mooring(anchors, length=L0, stiffness=k, damping=c)
    records, finals = {}, {}
    for name, go in (("resident", lambda s: s.run_resident(600, chunk=64)), ("eager", lambda s: s.run_eager(600)), ("never", lambda s: s.run_resident(600, chunk=64))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.set_sea(SeaState((0.5, 0.0, 0.0)))
        sim.set_mooring(anchors, length=L0, stiffness=k, damping=c)
        if name != "never":
            view = sim.track_extremes()
            assert view is sim.extremes and tuple(view.buffer.shape) == (1, 8, 64)
        rows = sim.record(list(range(64)), every=1, rows=600, wrench=True) if name == "resident" else None
        go(sim)
        finals[name] = sim.state()
        if name != "never":
            records[name] = view.bodies()
            if name == "resident":
                reach, peak = view.excursion(anchors[:, 0:2]), view.tension_max()
                states = rows.states()
                sim.stop_recording()
                sim.clear_extremes()
                assert sim.extremes is None
                sim.run_resident(64)
                assert _eq(view.bodies(), records[name])         # no longer updated
                assert sim.track_extremes() is view
        sim.close()
    assert _eq(records["resident"], records["eager"])
    assert _eq(finals["resident"], finals["eager"]) and _eq(finals["resident"], finals["never"])         # nothing feeds back
    r, s = records["resident"], finals["resident"]
    assert (r[:, ex.X_MIN] == sc.state[:, 0]).all() and (r[:, ex.X_MAX] >= s[:, 0]).all() and (r[:, ex.X_MAX] > r[:, ex.X_MIN] + 1.0).all()
    assert (r[:, ex.Z_MIN] <= s[:, 2]).all() and (r[:, ex.Z_MAX] >= s[:, 2]).all() and (r[:, ex.SPEED2_MAX] > 0).all()
    assert _eq(r[:, 0:7], Extremes.fold(states, np.zeros((600, 64), np.float32), ex.seed_of(sc.state))[:, 0:7])
    # the tension of step j + 1 is formed from the state of row j (step 1 from the initial state): the largest along the run
    along = np.stack([lines.tension(x) for x in [sc.state.astype(np.float64), *states[:-1].astype(np.float64)]]).max(axis=0)
    assert (peak > 0).all() and np.abs(peak - along).max() < 0.1, np.abs(peak - along).max()
    print(f"[64 moored buoys, 600 steps] peak tension {peak.min():.1f} .. {peak.max():.1f} N  watch circle {reach.min():.3f} .. {reach.max():.3f} m")
    assert (reach > 1.9).all() and (reach < 10.0).all()


def test_mooring_design_loads_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "mooring_design_loads.py"), "--steps", "256"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    peaks = [float(x) for x in re.findall(r"peak tension\s+([\d.]+) N", res.stdout)]
    assert len(peaks) == 9 and sum(p > 0.0 for p in peaks) >= 3, res.stdout      # the three pretensioned classes pull from the first step
