"""Mooring lines on the device (hydro_mooring_wrench, hydro_step_fused_tiled_multi_moor): without a record, and with a record
of all-zero k and c, the entry is the bed entry bit for bit; the probe follows the fp64 restatement of
tests/mooring_reference.py; a mooring step is, bit for bit, the bed entry's step given the probe's wrench as a world-frame
applied wrench; with implicit drag, applied wrench, pose hold, sea and bed it follows the fp64 step within the project's own
bound; a launch of 7 steps equals 7 of 1 and (2, 5), recorded rows included; refusals and guard bands; ClosedLoopSim's three
runners and a graph replay; the buoy of tests/test_mooring.py settles and keeps station on the device; the example.

Sizes: n = 200 (one block: three full tiles and 8 lanes) and n = 321 (two blocks, the last wave with one live lane).  The
population is mooring_population.line_population over the bodies of tests/test_seabed_gpu.py.

THE PROBE BOUND.  Errors of hydro_mooring_wrench against mooring_reference.wrench (fp64), in units of 2^-24 of
mooring_reference.wrench_scales, over the designed population, the eight bodies at the tie aside.  The rule: the next power
of two at or above twice the largest ratio measured.  PROBE_BOUND = 2 stands on the same arithmetic emulated on the host in
fp32 over this population (mooring_reference.wrench_fp32_emulated: the header's order, a correctly rounded seed for the
reciprocal square root): force 0.77, torque 0.33; 2 x 0.77 = 1.54.  On an MI355X: force 0.77, torque 0.28 (f32 and
f16 coefficients alike), the ties without a damper 0.05; 2 x 0.77 = 1.54.  The test prints the device's figures.

THE COMPOSITION OVER A BED.  The kernel adds the bed's wrench and then the line's: (h + W_bed) + W_line.  The bed entry given
W_line as an applied wrench adds (h + W_line) + W_bed - another rounding for a body that both touches the bed and pulls on
its line, so bit equality with that launch is asked of the bodies for which at most one of the two contributes.  For all
bodies the step over the bed equals, bit for bit, the mooring entry's step WITHOUT a bed given the bed's probe as the applied
wrench (the same two additions in the same order), and the recorded wrench of every body equals fl(fl(h + W_bed) + W_line)
formed on the host in fp32 from three device results.

Bound of the fp64 step comparison: integrator_oracle.STEP_ULP_BOUND (24), scales as in tests/test_seabed_gpu.py with the
line's own term magnitudes (mooring_reference.wrench_scales) added to the surrogate wrench."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mooring_reference as mr
import seabed_reference as br
import sea_reference as sr
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.mooring import Mooring
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop, SEA, SIZES, STEPS  # noqa: F401  (fixtures are requested by name)
from mooring_population import ALL_TILE, _buoys, CLAMPED, DEPTH, moored_pop as pop, NONE_TILE, OFF_TIES, population_report, TIES  # noqa: F401  (fixtures are requested by name)
from mooring_reference import PROBE_BOUND
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, raw, RHO, S_A,
                              S_C, S_IN, S_M, S_OUT, S_PV, S_PVO, _same, _same_bits, step, _tiled, _unguard, _untouched, _watched)

pytestmark = pytest.mark.gpu
WATCH = (0, 5, 63, 64, 80, 130)                                   # the watched bodies, with the last one
S_W = 6 * 64 + 28                                                 # the probe's


def test_population_is_what_it_was_designed_to_be(pop):
    st, _, _, _, _, rec = pop
    pulling, slack, none, clamped = population_report(rec, st)
    emulated = mr.taut_fp32(rec, st)
    assert (emulated == mr.taut(rec, st))[OFF_TIES].all()
    for n in SIZES:
        assert pulling[:n].mean() >= 0.25 and slack[:n].mean() >= 0.25 and none[:n].mean() >= 0.25, n
    assert none[64 * NONE_TILE:64 * NONE_TILE + 64].all() and mr.taut(rec, st)[64 * ALL_TILE:64 * ALL_TILE + 64].all()
    assert pulling[320] and clamped[CLAMPED].all() and clamped.sum() >= 8
    assert not rec[TIES[:4], 8].any() and (rec[TIES[4:], 8] > 0).all()


# ---- 1. no record, and a record without lines --------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_no_record_and_no_lines_are_the_bed_entry(coeff, implicit, pop, native_built):
    """mooring = NULL, and a record whose k and c are all zero (anchors, fairleads and lengths as drawn): the bits of
    hydro_step_fused_tiled_multi_bed - state, prev_out, kinetic energy and the recorded state and wrench - with and without
    log, applied wrench, control, sea and bed."""
    st, pv, params, applied, ctl, rec = pop
    unmoored = rec.copy()
    unmoored[:, 7:9] = 0.0
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)
        a, c17, none = _tiled(applied[:n]), _tiled(ctl[:n]), _tiled(unmoored[:n])
        combos = [(steps, app, control, with_log) for steps in STEPS for app in (None, a) for control in (None, c17) for with_log in (False, True)]

        def logs(with_log):
            return dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if with_log else {}
        for sea in (None, SEA):
            for bed in (None, BED):
                eng.set_sea(sea)
                eng.set_seabed(bed)
                for steps, app, control, with_log in combos:
                    cur, old = _buffers(st, pv, n)
                    w_ke, kw = _ke(), logs(with_log)
                    w_state, w_prev = step(eng, "bed", cur, old, n, steps, step0=3, control=control, applied=app, implicit=implicit, ke=w_ke, **kw)
                    w_log = kw.get("log")
                    for lines in (None, none):
                        c, o = _buffers(st, pv, n)
                        ke, kw = _ke(), logs(with_log)
                        got, got_prev = step(eng, "moor", c, o, n, steps, step0=3, mooring=lines, control=control, applied=app, implicit=implicit, ke=ke, **kw)
                        torch.cuda.synchronize()
                        what = (n, steps, app is None, control is None, with_log, sea is None, bed is None, lines is None)
                        assert _same_bits(got, w_state) and _same_bits(got_prev, w_prev) and _same_bits(ke, w_ke), what
                        assert not with_log or _same_bits(kw["log"], w_log), what
        eng.close()


# ---- 2. the probe ------------------------------------------------------------------------------------------------------------------
@COEFFS
def test_probe_against_the_fp64_restatement(coeff, pop, native_built):
    st, _, params, _, _, rec = pop
    worst = {"force": 0.0, "torque": 0.0, "ties with c = 0": 0.0}
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        got = _from(eng.mooring_wrench(_tiled(st[:n]), _tiled(rec[:n]), n), n)
        s, m, off = st[:n], rec[:n], OFF_TIES[:n]
        on = mr.taut(m, s)
        ref, scale = mr.wrench(m, s, on), mr.wrench_scales(m, s, on)
        live = (mr.tension(m, s, on) > 0) & off
        idle = ~live & off
        assert np.isfinite(got).all()
        assert not got[idle].any() and not np.signbit(got[idle]).any() and idle.sum() >= n // 2          # +0 where the line adds nothing
        assert (got[live, 0:3] != 0).any(axis=1).all() and live.sum() >= n // 4
        err = np.abs(got[live] - ref[live]) / (mr.ULP * scale[live])
        worst["force"] = max(worst["force"], float(err[:, 0:3].max()))
        worst["torque"] = max(worst["torque"], float(err[:, 3:6].max()))
        # the ties.  c = 0: T is continuous through x = 0, so either decision stands within the bound of the fp64 value
        everyone = np.ones(n, bool)
        tie_scale = mr.wrench_scales(m, s, contributing=everyone)
        t0, t1 = TIES[:4], TIES[4:]
        err0 = np.abs(got[t0] - ref[t0]) / (mr.ULP * tie_scale[t0])
        worst["ties with c = 0"] = max(worst["ties with c = 0"], float(err0.max()))
        # c > 0: the damper comes in at full strength at x = 0: the taut value or nothing
        taut_ref = mr.wrench(m, s, everyone)
        for b in t1:
            as_taut = (np.abs(got[b] - taut_ref[b]) <= PROBE_BOUND * mr.ULP * tie_scale[b]).all()
            assert as_taut or not got[b].any(), (b, got[b], taut_ref[b])
            assert taut_ref[b, 0:3].any()                        # (and the taut value is a force: the fairlead runs away)
        eng.close()
    print(f"[mooring probe, {coeff}] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {PROBE_BOUND:g})")
    assert max(worst.values()) <= PROBE_BOUND, worst


# ---- 3. a mooring step is the bed entry's step with the probe's wrench applied ---------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
@pytest.mark.parametrize("moving", [False, True], ids=["still", "sea"])
@pytest.mark.parametrize("with_bed", [False, True], ids=["nobed", "bed"])
def test_mooring_step_is_the_bed_step_with_the_probe_wrench_applied(coeff, semantics, implicit, moving, with_bed, pop, native_built):
    st, pv, params, _, _, rec = pop
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1]) if moving else None
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea(sea)
        eng.set_watch(list(range(n)))                            # every body's wrench is recorded
        lines = _tiled(rec[:n])
        probe = eng.mooring_wrench(_tiled(st[:n]), lines, n)
        w_line = _from(probe, n)
        pulls = w_line.any(axis=1)
        assert pulls.mean() > 0.25 and not pulls.all()

        def one(mooring, applied, bed, entry):
            eng.set_seabed(bed)
            log = torch.full((1, 19, n), NAN, dtype=torch.float32, device=DEV)
            cur, old = _buffers(st, pv, n)
            state, prev = step(eng, entry, cur, old, n, 1, step0=7, mooring=mooring, applied=applied, implicit=implicit, log=log)
            torch.cuda.synchronize()
            return state.clone(), prev.clone(), log

        bed = BED if with_bed else None
        got = one(lines, None, bed, "moor")
        want = one(None, probe, bed, "bed")                      # the bed entry given W as a world-frame applied wrench
        if not with_bed:
            assert all(_same_bits(x, y) for x, y in zip(got, want)), n
        else:
            eng.set_seabed(BED)
            w_bed = _from(eng.seabed_wrench(_tiled(st[:n]), n), n)
            touches = w_bed.any(axis=1)
            both = touches & pulls
            assert both.sum() >= 8 and (touches & ~pulls).sum() >= 8 and (pulls & ~touches).sum() >= 8
            g_state, w_state = _from(got[0], n), _from(want[0], n)
            assert np.array_equal(g_state[~both].view(np.uint32), w_state[~both].view(np.uint32)), n
            g_log, w_log = got[2][0].cpu().numpy().T, want[2][0].cpu().numpy().T                       # (n, 19)
            assert np.array_equal(g_log[~both].view(np.uint32), w_log[~both].view(np.uint32)), n
            # all bodies: the same two additions in the same order, the bed's wrench arriving as the applied one
            chained = one(lines, _tiled(w_bed), None, "moor")
            assert all(_same_bits(x, y) for x, y in zip(got, chained)), n
            # and the recorded wrench is fl(fl(h + W_bed) + W_line)
            h = one(None, None, None, "bed")[2][0].cpu().numpy().T[:, 13:19]
            total = np.where(touches[:, None], h + w_bed, h)
            total = np.where(pulls[:, None], total + w_line, total)
            assert total.dtype == np.float32 and np.array_equal(g_log[:, 13:19], total), n
        eng.close()


# ---- 4. everything together against fp64 ---------------------------------------------------------------------------------------------
@COEFFS
def test_one_step_with_everything_against_fp64(coeff, pop, native_built):
    """Implicit drag + applied wrench + pose hold + sea + bed + lines.  Reference: integrator_oracle.integrate of the TRUE state
    with (the device's hydrodynamic wrench of the host-built relative state + applied + the pose-hold law + the fp64 bed wrench
    + the fp64 line wrench of the TRUE state), drag_jacobian of the relative state.  Bodies within 1e-4 of a branch of the
    hydrodynamic model in the relative state are left out, as in tests/test_sea_gpu.py, and the four ties with a damper."""
    st, pv, params, applied, ctl, rec = pop
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        w = _from(eng.sea_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        keep[TIES[4:]] = False
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step(eng, "moor", cur, old, n, 1, step0=7, mooring=_tiled(rec[:n]), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        on = mr.taut_fp32(rec[:n], st[:n])
        extra = br.wrench(BED, st[:n], pr[:n], touch) + mr.wrench(rec[:n], st[:n], on)
        extra_scale = br.wrench_scales(BED, st[:n], pr[:n], touch) + mr.wrench_scales(rec[:n], st[:n], on)
        assert (mr.tension(rec[:n], st[:n], on)[keep] > 0).mean() > 0.25
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=extra[keep], bed_scale=extra_scale[keep])
        eng.close()
    from oracle import integrator_oracle as io
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[sea + applied + pose hold + bed + lines, implicit, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g})")
    assert max(per_group.values()) <= B, worst


# ---- 5. step counts and the recorder -----------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    """7 steps = 7 x 1 = (2, 5) with step0 advanced: state, prev_out and every recorded row (state and wrench) of the watched
    bodies - moored and pulling ones among them."""
    st, pv, params, _, _, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)
        assert (mr.tension(rec[:n], st[:n])[watched] > 0).sum() >= 2
        lines = _tiled(rec[:n])

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                step(eng, "moor", cur, old, n, k, step0=100 + done, mooring=lines, implicit=implicit, log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, old[:, 7:13], log
        one, singles, chunks = run([7]), run([1] * 7), run([2, 5])
        for other in (singles, chunks):
            assert all(_same_bits(x, y) for x, y in zip(one, other)), n
        assert not implicit or not torch.isnan(one[2]).any()
        eng.close()


@COEFFS_SEMANTICS
@DRAG
def test_energy_and_non_temporal_instantiations_with_lines_pulling(coeff, semantics, implicit, pop, native_built):
    """The instantiations the tests above do not launch with lines that pull: KE = true (the state bits of the launch without
    sampling, and with implicit drag the energy pair of the returned state against scenes.kinetic_energy_fp64 to 1e-12, with
    and without the rotational term) and NT = true (set_tuning(0, 0, 1): the bits of the temporal launch), with sea, bed, pose hold and
    applied wrench active."""
    st, pv, params, applied, ctl, rec = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines, a, c17 = _tiled(rec[:n]), _tiled(applied[:n]), _tiled(ctl[:n])

        def run(ke=None, **kw):
            cur, old = _buffers(st, pv, n)
            state, prev = step(eng, "moor", cur, old, n, 7, step0=5, mooring=lines, control=c17, applied=a, implicit=implicit, ke=ke, **kw)
            torch.cuda.synchronize()
            return state, prev
        eng.set_tuning(0, 0, 0)
        want = run()
        for rotational in (True, False):
            ke = _ke()
            got = run(ke, rotational=rotational)
            assert all(_same_bits(x, y) for x, y in zip(got, want)), (n, rotational)
            state, pair = _from(got[0], n), ke.cpu().tolist()
            if implicit:                                         # (seven explicit steps may carry a light body out of range)
                assert np.isfinite(state).all(), (n, rotational)
                lin, rot = scenes.kinetic_energy_fp64(state, params[coeff][:n], rotational=True)
                assert lin > 0 and rot > 0 and pair[0] == pytest.approx(lin, rel=1e-12), (n, rotational, pair, lin)
                assert (pair[1] == pytest.approx(rot, rel=1e-12)) if rotational else pair[1] == 0.0, (n, rotational, pair, rot)
        eng.set_tuning(0, 0, 1)
        ke_t, ke_nt = _ke(), _ke()
        streamed = run()
        assert all(_same_bits(x, y) for x, y in zip(streamed, want)), n
        streamed = run(ke_nt)
        eng.set_tuning(0, 0, 0)
        run(ke_t)
        assert all(_same_bits(x, y) for x, y in zip(streamed, want)) and _same_bits(ke_nt, ke_t), n
        eng.close()


# ---- 6. refusals and guards through the raw C ABI ------------------------------------------------------------------------------------


def test_refusals_launch_nothing(pop, native_built):
    """The refusals are the bed entry's, in its order, then the mooring's; the probe's own.  Nothing is written."""
    st, pv, params, applied, ctl, rec = pop
    n = 321
    eng = _engine(n, params["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a, c17, m9 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C), _guarded(rec[:n], S_M)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    m = m9.data_ptr()
    for bed, sea in ((BED, None), (BED, SEA), (None, None)):
        eng.set_watch(None)
        eng.set_seabed(bed)
        eng.set_sea(sea)
        for lines in (m, None):                                  # the bed entry's refusals, with lines and without
            assert raw(eng, "moor", n, state, prev, out, pvo, step0=-1, mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, step0=2 ** 52 - 1, mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, steps=0, mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, applied=a.data_ptr() + 4, mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, control=c17.data_ptr() + 4, mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, control=out.data_ptr(), mooring=lines) == (E_ARG, -7)
            assert raw(eng, "moor", n, state, prev, out, pvo, log=log, mooring=lines) == (E_STATE, -7)        # a log without a watch list
        # the mooring's own
        assert raw(eng, "moor", n, state, prev, out, pvo, mooring=m + 4) == (E_ARG, -7)                       # misaligned
        assert raw(eng, "moor", n, state, prev, out, pvo, mooring=m, s_mooring=572) == (E_ARG, -7)               # below 9 * 64
        assert raw(eng, "moor", n, state, prev, out, pvo, mooring=m, s_mooring=578) == (E_ARG, -7)               # not a multiple of 4
        assert raw(eng, "moor", n, state, prev, out, pvo, mooring=out.data_ptr()) == (E_ARG, -7)              # aliases state_out
        assert raw(eng, "moor", n, state, prev, out, pvo, mooring=pvo.data_ptr()) == (E_ARG, -7)              # aliases prev_out
        assert "mooring must not overlap" in eng._lib.hydro_last_error(eng._h).decode()
        # control is refused before the mooring
        assert raw(eng, "moor", n, state, prev, out, pvo, control=c17.data_ptr() + 4, mooring=m + 4) == (E_ARG, -7)
        assert "mooring" not in eng._lib.hydro_last_error(eng._h).decode()
        eng.set_watch([0, 320])
        assert raw(eng, "moor", n, state, prev, out, pvo, steps=5, log=log, mooring=m) == (E_ARG, -7)          # rows 0 .. 4 of 4
        assert raw(eng, "moor", n, state, prev, out, pvo, log=log, mooring=log.data_ptr()) == (E_ARG, -7)     # aliases the log
    # the probe
    lib, s = eng._lib, eng._stream(None)
    sp, wp = state.data_ptr(), w.data_ptr()
    for args in ((n, None, S_IN, m, S_M, wp, S_W), (n, sp, S_IN, None, S_M, wp, S_W), (n, sp, S_IN, m, S_M, None, S_W),
                 (n, sp + 4, S_IN, m, S_M, wp, S_W), (n, sp, S_IN, m + 4, S_M, wp, S_W), (n, sp, S_IN, m, S_M, wp + 4, S_W),
                 (n, sp, 828, m, S_M, wp, S_W), (n, sp, S_IN, m, 572, wp, S_W), (n, sp, S_IN, m, S_M, wp, 380),
                 (n + 1, sp, S_IN, m, S_M, wp, S_W), (-1, sp, S_IN, m, S_M, wp, S_W),
                 (n, sp, S_IN, m, S_M, sp, S_W), (n, sp, S_IN, m, S_M, m, S_W), (n, sp, S_IN, wp, S_M, wp, S_W)):       # out overlaps an input
        assert lib.hydro_mooring_wrench(eng._h, *args, s) == E_ARG, args
    bare = type(eng)(n, DEV, RHO, G)                              # no parameters yet
    assert lib.hydro_mooring_wrench(bare._h, n, sp, S_IN, m, S_M, wp, S_W, bare._stream(None)) == E_STATE
    bare.close()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all() and torch.isnan(w).all()
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or overwritten - state_out,
    prev_out, log and the probe's out - and the inputs are untouched."""
    st, pv, params, applied, ctl, rec = pop
    n, tiles = 200, 4
    eng = _engine(n, params[coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    state, prev, a, c17, m9 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C), _guarded(rec[:n], S_M)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    eng._check(eng._lib.hydro_mooring_wrench(eng._h, n, state.data_ptr(), S_IN, m9.data_ptr(), S_M, w.data_ptr(), S_W, eng._stream(None)))
    rc, written = raw(eng, "moor", n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, log=log, applied=a.data_ptr(), control=c17.data_ptr(), mooring=m9.data_ptr())
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    line, wrest = _unguard(w, n, 6, S_W)
    assert np.isnan(rest).all() and np.isnan(prest).all() and np.isnan(wrest).all(), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9), before))
    assert np.isfinite(line).all(), "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want, want_prev = step(eng, "moor", cur, old, n, 3, step0=11, mooring=_tiled(rec[:n]), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint32), _from(want, n).view(np.uint32))
    assert np.array_equal(pv_out.view(np.uint32), _from(want_prev, n).view(np.uint32))
    assert np.array_equal(line.view(np.uint32), _from(eng.mooring_wrench(_tiled(st[:n]), _tiled(rec[:n]), n), n).view(np.uint32))
    eng.close()


# ---- 7. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 321), each on a line of its own: the anchor 5 m from the body in a drawn direction, 4.9 m of line,
    the default constants for its mass."""
    sc = scenes.scene_c2(n=321)
    rng = np.random.default_rng(5)
    d = rng.normal(size=(sc.n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k, c = Mooring.for_body(sc.params[:, 10].astype(np.float64), sc.dt)
    lines = dict(anchor=sc.state[:, 0:3].astype(np.float64) + 5.0 * d, fairlead=(0.05, 0.0, -0.05), length=4.9, stiffness=k, damping=c)
    return sc, lines


def test_sim_runners_agree_with_lines_set(native_built):
    sc, lines = _scene()
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        buf = sim.set_mooring(**lines)
        assert buf is sim.mooring and tuple(buf.shape) == (6, 9, 64)
        go(sim)
        assert name != "graph" or sim._graph is not None
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc, implicit_drag=True)
    plain.run_resident(64)
    for name in ("resident", "chunks", "graph"):
        assert _same(finals["eager"], finals[name]), name
    free = plain.state()
    assert (np.linalg.norm(finals["eager"][:, 0:3] - free[:, 0:3], axis=1) > 1e-3).mean() > 0.9          # the lines pulled
    plain.close()


def test_graph_replays_with_lines_bed_and_current_and_clear_mooring(native_built):
    sc, lines = _scene()
    bed, current = Seabed.for_step(-30.0, sc.dt), SeaState((0.4, -0.1, 0.0))
    g, r, never, cleared = (ClosedLoopSim(sc, implicit_drag=True) for _ in range(4))
    for s in (g, r):
        s.set_sea(current)
        s.set_seabed(bed)
        s.set_mooring(**lines)
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state())
    never.run_resident(64)
    assert not np.array_equal(r.state(), never.state())
    cleared.set_mooring(**lines)
    cleared.clear_mooring()
    assert cleared.mooring is None
    cleared.run_resident(32)
    cleared.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state())
    waves = ClosedLoopSim(sc, implicit_drag=True)
    waves.set_mooring(**lines)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_mooring(**lines)
    for s in (g, r, never, cleared, waves, two_kernel):
        s.close()


# ---- 8. the buoy of tests/test_mooring.py on the device ---------------------------------------------------------------------------------


def test_still_water_the_buoys_settle_at_the_analytic_depth_on_the_device(native_built):
    sc, anchors, z_eq, mass = _buoys()
    k, c = Mooring.for_body(mass, sc.dt)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_mooring(anchors, length=DEPTH - 1.0, stiffness=k, damping=c)
    sim.run_resident(1800, chunk=64)
    s = sim.state().astype(np.float64)
    z_want = (sc.rho * sc.g * 0.5 - mass * sc.g - k * (DEPTH - z_eq - (DEPTH - 1.0))) / (sc.rho * sc.g + k)
    lines = Mooring(anchors, length=DEPTH - 1.0, stiffness=k, damping=c)
    T = lines.tension(s)
    speed = np.linalg.norm(s[:, 7:10], axis=1)
    print(f"[still water on the device] |v| <= {speed.max():.2e} m/s  z {s[:, 2].min():+.6f} .. {s[:, 2].max():+.6f} m (analytic {z_want:+.6f})  "
          f"T {T.min():.2f} .. {T.max():.2f} N")
    assert speed.max() < 1e-5 and np.abs(s[:, 2] - z_want).max() < 1e-4
    assert np.abs(T - (sc.rho * sc.g * (0.5 - s[:, 2]) - mass * sc.g)).max() < 0.1
    sim.close()


def test_current_the_buoys_keep_station_on_the_device(native_built):
    sc, anchors, z_eq, mass = _buoys()
    k, c = Mooring.for_body(mass, sc.dt)
    L0 = DEPTH + 0.5
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(SeaState((0.5, 0.0, 0.0)))
    sim.set_mooring(anchors, length=L0, stiffness=k, damping=c)
    sim.run_resident(2999, chunk=64)
    rec = sim.record(list(range(64)), every=1, rows=601, wrench=True)
    sim.run_resident(601, chunk=64)
    states, wrenches = rec.states().astype(np.float64), rec.wrenches().astype(np.float64)                # (601, 64, 13), (601, 64, 6)
    lines = Mooring(anchors, length=L0, stiffness=k, damping=c)
    # row j + 1 holds the wrench formed from the state of row j: the line's share of it by the fp64 restatement
    line_fx = np.stack([lines.wrench(states[j])[:, 0] for j in range(600)])
    tension = np.stack([lines.tension(states[j]) for j in range(600)])
    reach = np.stack([lines.geometry(states[j])[2] for j in range(600)])
    hydro_fx = wrenches[1:, :, 0] - line_fx
    offset = states[:, :, 0] - anchors[None, :, 0]
    print(f"[current on the device] x - x_anchor {offset[-1].min():.3f} .. {offset[-1].max():.3f} m  T {tension.mean(axis=0).min():.1f} .. "
          f"{tension.mean(axis=0).max():.1f} N  line F_x {line_fx.mean(axis=0).min():.2f} .. {line_fx.mean(axis=0).max():.2f} N  "
          f"hydrodynamic f_x {hydro_fx.mean(axis=0).min():.2f} .. {hydro_fx.mean(axis=0).max():.2f} N")
    assert reach.max() < 1.01 * L0
    assert (hydro_fx.mean(axis=0) > 50.0).all() and (np.abs(-line_fx.mean(axis=0) - hydro_fx.mean(axis=0)) <= 0.05 * hydro_fx.mean(axis=0)).all()
    assert (tension > 0).all()                                   # never slack there
    adrift = ClosedLoopSim(sc, implicit_drag=True)
    adrift.set_sea(SeaState((0.5, 0.0, 0.0)))
    adrift.run_resident(3600, chunk=64)
    assert ((adrift.state()[:, 0] - anchors[:, 0]) > 20.0).all()
    for s in (sim, adrift):
        s.close()


def test_moored_buoy_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "moored_buoy.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    m = re.search(r"mean tension ([\d.]+) N", res.stdout)
    assert m and float(m.group(1)) > 0.0, res.stdout
