"""Tethers on the device (hydro_tether_wrench, hydro_step_fused_tiled_multi_teth): the probe's forces are equal and opposite
bit for bit and follow the fp64 restatement of tests/tether_reference.py; without a record, and with a record of zeros, the
entry is the extremes entry bit for bit; a tether step is, bit for bit, the extremes entry's step given the probe's wrench as
a world-frame applied wrench; with implicit drag, applied wrench, pose hold, sea, bed and mooring lines it follows the fp64
step within the project's own bound; a launch of 7 steps equals 7 of 1 and (2, 5), recorded rows included; the KE and NT
instantiations; refusals and guard bands; ClosedLoopSim's three runners and a graph replay; the hanging pair of
tests/test_tether.py on the device; the example.

Sizes: n = 200 (one block: three full tiles and 8 lanes), n = 321 (two blocks, the last wave with one live lane, which has no
tether) and n = 322 (the last wave's two live lanes are a pair).  The population is tether_population.tether_population over the
bodies of tests/test_seabed_gpu.py and one more; the mooring lines are those of tests/test_mooring.py.

THE PROBE BOUND.  Errors of hydro_tether_wrench against tether_reference.wrench (fp64), in units of 2^-24 of
tether_reference.wrench_scales, over the designed population, the sixteen bodies at the tie aside.  PROBE_BOUND = 2
(tests/test_tether.py: the header's order emulated on the host in fp32, force 0.90, torque 0.48, tension 0.90; 2 x 0.90 =
1.80).  The test prints the device's figures; profiles/tether.json and DESIGN.md section 22 record them.

THE COMPOSITION WITH A BED OR A MOORING LINE.  The kernel adds the bed's wrench, the mooring line's and then the tether's:
((h + W_bed) + W_moor) + W_teth.  The extremes entry given W_teth as an applied wrench adds ((h + W_teth) + W_bed) + W_moor -
other roundings for a body that is pulled by its tether AND touches the bed or is pulled by its mooring line, so bit equality
with that launch is asked of the bodies for which the tether or neither of the other two contributes: the additions compared
are h + W_teth (tether alone), (h + W_bed) + W_moor (no tether) and h alone.  For ALL bodies the step over the bed (or with the
mooring lines) equals, bit for bit, the tether entry's step WITHOUT it given its probe as the applied wrench: (h + W_bed) +
W_teth and (h + W_moor) + W_teth, the same two additions in the same order.

Bound of the fp64 step comparison: integrator_oracle.STEP_ULP_BOUND (24), scales as in tests/test_mooring_gpu.py with the
tether's own term magnitudes (tether_reference.wrench_scales) added to the surrogate wrench."""
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
import tether_reference as tr
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from silver2_isaacsim_amd.tether import Tether
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, raw, RHO, S_A,
                              S_C, S_IN, S_M, S_OUT, S_PV, S_PVO, _same, _same_bits, step, _tiled, _unguard, _untouched)
from tether_population import (assert_antisymmetric, bodies_of, check_population, designed_population, hanging_pair, LINE, record_for, SIZES, tether_population)
from tether_reference import PROBE_BOUND

pytestmark = pytest.mark.gpu
STEPS = (1, 7)
S_E = 8 * 64 + 36                                                 # the extremes record's
S_T = 7 * 64 + 44                                                 # the tether record's
S_W = 6 * 64 + 28                                                 # the probe's wrench
S_T1 = 64 + 12                                                    # the probe's tension


@pytest.fixture(scope="module")
def pop(bed_pop, hold_pop):
    """The 321 bodies of tests/test_seabed_gpu.py and body 321 of the population they were drawn from, with the tethers of
    tether_population.tether_population and the mooring lines of mooring_population.line_population (body 321 has none)."""
    st, pv, params, applied, ctl = bed_pop
    more = hold_pop
    cat = lambda a, b: np.concatenate([a, b[321:322]])  # noqa: E731
    st, pv, applied, ctl = cat(st, more[0]), cat(pv, more[1]), cat(applied, more[3]), cat(ctl, more[4])
    params = {k: cat(params[k], more[2][k]) for k in params}
    st, pv, rec, groups = tether_population(st, pv, params["f32"])
    moor = np.concatenate([line_population(st[:321], params["f32"][:321]), np.zeros((1, 9), np.float32)])
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, rec=rec, groups=groups, moor=moor,
                ties=bodies_of(groups, "ties_0", "ties_c"))


def test_population_is_what_it_was_designed_to_be(pop):
    check_population(pop["st"], pop["rec"], pop["groups"])
    st, _, _, rec, _ = designed_population()                      # and it is the one tests/test_tether.py derives the bound on
    assert np.array_equal(st, pop["st"]) and np.array_equal(rec, pop["rec"])


def _probe(eng, st, rec, n):
    """(W (n, 6), T (n,), the tiled W) of hydro_tether_wrench."""
    tension = eng.alloc_tiled(1, n)
    w = eng.tether_wrench(_tiled(st[:n]), _tiled(rec), n, tension=tension)
    return _from(w, n), _from(tension, n)[:, 0], w


# ---- 1. the probe ------------------------------------------------------------------------------------------------------------------
def test_probe_forces_are_equal_and_opposite_bit_for_bit(pop, native_built):
    """F_i == -F_j and T_i == T_j for every pair - the ties, the clamped and the coincident pair included, across lanes 31 | 32,
    between lanes 0 and 63 - and +0 wherever the line adds nothing."""
    for n in SIZES:
        eng = _engine(n, pop["params"]["f32"], "f32")
        rec = record_for(pop["rec"], n)
        W, T, _ = _probe(eng, pop["st"], rec, n)
        assert np.isfinite(W).all() and np.isfinite(T).all()
        assert assert_antisymmetric(W, T, rec) >= n // 4
        without = _from(eng.tether_wrench(_tiled(pop["st"][:n]), _tiled(rec), n), n)               # tension = NULL: the same W
        assert np.array_equal(without.view(np.uint32), W.view(np.uint32))
        eng.close()


def test_probe_against_the_fp64_restatement(pop, native_built):
    st, groups, ties = pop["st"], pop["groups"], pop["ties"]
    worst = {"force": 0.0, "torque": 0.0, "tension": 0.0, "ties with c = 0": 0.0}
    for n in SIZES:
        eng = _engine(n, pop["params"]["f32"], "f32")
        t, s = record_for(pop["rec"], n), st[:n]
        got, got_T, _ = _probe(eng, st, t, n)
        off = ~np.isin(np.arange(n), ties)
        on = tr.taut(t, s)
        ref, scale, ref_T, scale_T = tr.wrench(t, s, on), tr.wrench_scales(t, s, on), tr.tension(t, s, on), tr.tension_scale(t, s, on)
        live = (ref_T > 0) & off
        idle = ~live & off
        assert not got[idle].any() and not np.signbit(got[idle]).any() and not got_T[idle].any() and idle.sum() >= n // 2   # +0 where the line adds nothing
        assert (got[live, 0:3] != 0).any(axis=1).all() and (got_T[live] > 0).all() and live.sum() >= n // 4
        err = np.abs(got[live] - ref[live]) / (tr.ULP * scale[live])
        worst["force"] = max(worst["force"], float(err[:, 0:3].max()))
        worst["torque"] = max(worst["torque"], float(err[:, 3:6].max()))
        worst["tension"] = max(worst["tension"], float((np.abs(got_T[live] - ref_T[live]) / (tr.ULP * scale_T[live])).max()))
        # the ties.  c = 0: T is continuous through x = 0, so either decision stands within the bound of the fp64 value
        everyone = np.ones(n, bool)
        tie_scale = tr.wrench_scales(t, s, contributing=everyone)
        t0, t1 = bodies_of(groups, "ties_0"), bodies_of(groups, "ties_c")
        err0 = np.abs(got[t0] - ref[t0]) / (tr.ULP * tie_scale[t0])
        worst["ties with c = 0"] = max(worst["ties with c = 0"], float(err0.max()))
        # c > 0: the damper comes in at full strength at x = 0: the taut value or nothing
        taut_ref = tr.wrench(t, s, everyone)
        for b in t1:
            as_taut = (np.abs(got[b] - taut_ref[b]) <= PROBE_BOUND * tr.ULP * tie_scale[b]).all()
            assert as_taut or not got[b].any(), (b, got[b], taut_ref[b])
            assert taut_ref[b, 0:3].any()                        # (and the taut value is a force: the fairleads part)
        eng.close()
    print("[tether probe] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {PROBE_BOUND:g})")
    assert max(worst.values()) <= PROBE_BOUND, worst


# ---- 2. no record, and a record of zeros -----------------------------------------------------------------------------------------------
OPTIONS = ("log", "applied", "control", "sea", "bed", "mooring", "extremes")


@COEFFS
@DRAG
def test_no_record_and_a_record_of_zeros_are_the_extremes_entry(coeff, implicit, pop, native_built):
    """tether = NULL, and a record that is all zeros: the bits of hydro_step_fused_tiled_multi_ext - state, prev_out, kinetic
    energy, the recorded state and wrench and the extremes record - with none of log, applied wrench, control, sea, bed,
    mooring lines and extremes, with each of them alone, and with all of them."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        watched = sorted({b for b in (0, 5, 63, 64, 80, 130, n - 1) if b < n})
        eng.set_watch(watched)
        a, c17, m9, zeros = _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n]), _tiled(pop["moor"][:n]), _tiled(np.zeros((n, 7), np.float32))
        for chosen in [()] + [(o,) for o in OPTIONS] + [OPTIONS]:
            eng.set_sea(SEA if "sea" in chosen else None)
            eng.set_seabed(BED if "bed" in chosen else None)
            for steps in STEPS:
                def run(tether, entry):
                    cur, old = _buffers(st, pv, n)
                    ke = _ke()
                    kw = dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if "log" in chosen else {}
                    ext = eng.extremes_reset(eng.alloc_tiled(8, n), n) if "extremes" in chosen else None
                    state, prev = step(eng, entry, cur, old, n, steps, step0=3, tether=tether, extremes=ext, mooring=m9 if "mooring" in chosen else None,
                                       control=c17 if "control" in chosen else None, applied=a if "applied" in chosen else None, implicit=implicit, ke=ke, **kw)
                    torch.cuda.synchronize()
                    return [state, prev, ke] + ([kw["log"]] if kw else []) + ([ext] if ext is not None else [])
                want = run(None, "ext")
                for tether in (None, zeros):
                    got = run(tether, "teth")
                    assert all(_same_bits(x, y) for x, y in zip(got, want)), (n, steps, chosen, tether is None)
        eng.close()


# ---- 3. a tether step is the extremes entry's step with the probe's wrench applied -----------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
@pytest.mark.parametrize("moving", [False, True], ids=["still", "sea"])
@pytest.mark.parametrize("extra", ["none", "bed", "moor"])
def test_tether_step_is_the_extremes_step_with_the_probe_wrench_applied(coeff, semantics, implicit, moving, extra, pop, native_built):
    st, pv = pop["st"], pop["pv"]
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1]) if moving else None
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(sea)
        eng.set_watch(list(range(n)))                            # every body's wrench is recorded
        rec = record_for(pop["rec"], n)
        lines, m9 = _tiled(rec), _tiled(pop["moor"][:n])
        w_teth, _, probe = _probe(eng, st, rec, n)
        pulls = w_teth.any(axis=1)
        assert pulls.mean() > 0.25 and not pulls.all()

        def one(tether, applied, bed, mooring, entry):
            eng.set_seabed(bed)
            log = torch.full((1, 19, n), NAN, dtype=torch.float32, device=DEV)
            cur, old = _buffers(st, pv, n)
            state, prev = step(eng, entry, cur, old, n, 1, step0=7, tether=tether, mooring=mooring, applied=applied, implicit=implicit, log=log)
            torch.cuda.synchronize()
            return state.clone(), prev.clone(), log

        bed, moor = (BED if extra == "bed" else None), (m9 if extra == "moor" else None)
        got = one(lines, None, bed, moor, "teth")
        want = one(None, probe, bed, moor, "ext")                # the extremes entry given W as a world-frame applied wrench
        if extra == "none":
            assert all(_same_bits(x, y) for x, y in zip(got, want)), n
        else:
            if extra == "bed":
                eng.set_seabed(BED)
                w_other = _from(eng.seabed_wrench(_tiled(st[:n]), n), n)
            else:
                w_other = _from(eng.mooring_wrench(_tiled(st[:n]), m9, n), n)
            other = w_other.any(axis=1)
            both = other & pulls
            assert both.sum() >= 8 and (other & ~pulls).sum() >= 8 and (pulls & ~other).sum() >= 8
            g_state, w_state = _from(got[0], n), _from(want[0], n)
            assert np.array_equal(g_state[~both].view(np.uint32), w_state[~both].view(np.uint32)), n
            g_log, w_log = got[2][0].cpu().numpy().T, want[2][0].cpu().numpy().T                       # (n, 19)
            assert np.array_equal(g_log[~both].view(np.uint32), w_log[~both].view(np.uint32)), n
            # all bodies: the same two additions in the same order, the other wrench arriving as the applied one
            chained = one(lines, _tiled(w_other), None, None, "teth")
            assert all(_same_bits(x, y) for x, y in zip(got, chained)), n
            # and the recorded wrench is fl(fl(h + W_other) + W_teth)
            h = one(None, None, None, None, "ext")[2][0].cpu().numpy().T[:, 13:19]
            total = np.where(other[:, None], h + w_other, h)
            total = np.where(pulls[:, None], total + w_teth, total)
            assert total.dtype == np.float32 and np.array_equal(g_log[:, 13:19], total), n
        eng.close()


# ---- 4. everything together against fp64 ---------------------------------------------------------------------------------------------
@COEFFS
def test_one_step_with_everything_against_fp64(coeff, pop, native_built):
    """Implicit drag + applied wrench + pose hold + sea + bed + mooring lines + tethers.  Reference: integrator_oracle.integrate
    of the TRUE state with (the device's hydrodynamic wrench of the host-built relative state + applied + the pose-hold law +
    the fp64 bed, mooring and tether wrenches of the TRUE state), drag_jacobian of the relative state.  Bodies within 1e-4 of a
    branch of the hydrodynamic model in the relative state are left out, as in tests/test_sea_gpu.py, and the ties with a
    damper of either kind of line."""
    from mooring_population import TIES as MOOR_TIES
    st, pv, applied, ctl = pop["st"], pop["pv"], pop["applied"], pop["ctl"]
    pr = pop["params"][coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        rec, moor = record_for(pop["rec"], n), pop["moor"][:n]
        w = _from(eng.sea_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        keep[MOOR_TIES[4:]] = False
        keep[bodies_of(pop["groups"], "ties_c")] = False
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step(eng, "teth", cur, old, n, 1, step0=7, tether=_tiled(rec), mooring=_tiled(moor), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        on_m, on_t = mr.taut_fp32(moor, st[:n]), tr.taut_fp32(rec, st[:n])
        extra = br.wrench(BED, st[:n], pr[:n], touch) + mr.wrench(moor, st[:n], on_m) + tr.wrench(rec, st[:n], on_t)
        extra_scale = br.wrench_scales(BED, st[:n], pr[:n], touch) + mr.wrench_scales(moor, st[:n], on_m) + tr.wrench_scales(rec, st[:n], on_t)
        assert (tr.tension(rec, st[:n], on_t)[keep] > 0).mean() > 0.2
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=extra[keep], bed_scale=extra_scale[keep])
        eng.close()
    from oracle import integrator_oracle as io
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[sea + applied + pose hold + bed + lines + tethers, implicit, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g})")
    assert max(per_group.values()) <= B, worst


# ---- 5. step counts and the recorder -----------------------------------------------------------------------------------------------------
def _watched_pairs(pop, n):
    """Both bodies of pairs that pull - one across lanes 31 | 32, lanes 0 and 63 of tile 1, neighbours - and the last body."""
    tile0 = [int(b) for pair in pop["groups"]["pull"] if pair[0] < 64 for b in pair][:4]         # two pairs i <-> i + 32 that pull, over the bed
    return sorted({b for b in [64, 127, 95, 96, 200, 201, 202, 203, n - 2, n - 1] + tile0 if b < n})


@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    """7 steps = 7 x 1 = (2, 5) with step0 advanced: state, prev_out and every recorded row (state and wrench) of the watched
    bodies - both bodies of tethered pairs.  The partner's state of step k reaches a lane from inside the launch or from memory:
    the same bits."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        watched = _watched_pairs(pop, n)
        eng.set_watch(watched)
        rec = record_for(pop["rec"], n)
        assert (tr.tension(rec, st[:n])[watched] > 0).sum() >= 6
        lines, m9 = _tiled(rec), _tiled(pop["moor"][:n])

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                step(eng, "teth", cur, old, n, k, step0=100 + done, tether=lines, mooring=m9, implicit=implicit, log=log, every=1, phase=1, row0=done)
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
def test_energy_and_non_temporal_instantiations_with_tethers_pulling(coeff, semantics, implicit, pop, native_built):
    """KE = true (the state bits of the launch without sampling - the lanes past n are masked, not gone, in these - and with
    implicit drag the energy pair of the returned state against scenes.kinetic_energy_fp64 to 1e-12, with and without the
    rotational term) and NT = true (set_tuning(0, 0, 1): the bits of the temporal launch), with sea, bed, pose hold, applied
    wrench, mooring lines and extremes active."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines, m9, a, c17 = _tiled(record_for(pop["rec"], n)), _tiled(pop["moor"][:n]), _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n])

        def run(ke=None, **kw):
            cur, old = _buffers(st, pv, n)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            state, prev = step(eng, "teth", cur, old, n, 7, step0=5, tether=lines, extremes=ext, mooring=m9, control=c17, applied=a, implicit=implicit, ke=ke, **kw)
            torch.cuda.synchronize()
            return state, prev, ext
        eng.set_tuning(0, 0, 0)
        want = run()
        for rotational in (True, False):
            ke = _ke()
            got = run(ke, rotational=rotational)
            assert all(_same_bits(x, y) for x, y in zip(got, want)), (n, rotational)
            state, pair = _from(got[0], n), ke.cpu().tolist()
            if implicit:                                         # (seven explicit steps may carry a light body out of range)
                assert np.isfinite(state).all(), (n, rotational)
                lin, rot = scenes.kinetic_energy_fp64(state, pop["params"][coeff][:n], rotational=True)
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
    """The refusals are the extremes entry's, in its order, then the tether's; the probe's own.  Nothing is written."""
    n = 322
    st, pv = pop["st"], pop["pv"]
    eng = _engine(n, pop["params"]["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m9, t7 = _guarded(pop["moor"][:n], S_M), _guarded(record_for(pop["rec"], n), S_T)
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    w1 = torch.full((tiles * S_T1,), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    t, m, e = t7.data_ptr(), m9.data_ptr(), e8.data_ptr()
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    for bed, sea in ((BED, None), (BED, SEA), (None, None)):
        eng.set_watch(None)
        eng.set_seabed(bed)
        eng.set_sea(sea)
        for lines in (t, None):                                  # the extremes entry's refusals, with tethers and without
            assert raw(eng, "teth", n, state, prev, out, pvo, step0=-1, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, step0=2 ** 52 - 1, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, steps=0, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, applied=a.data_ptr() + 4, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, control=c17.data_ptr() + 4, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, control=out.data_ptr(), s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, mooring=m + 4, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, mooring=m, extremes=e + 4, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)
            assert raw(eng, "teth", n, state, prev, out, pvo, extremes=state.data_ptr(), s_extremes=S_E, tether=lines, s_tether=S_T) == (E_ARG, -7)     # extremes over an input
            assert raw(eng, "teth", n, state, prev, out, pvo, log=log, s_extremes=S_E, tether=lines, s_tether=S_T) == (E_STATE, -7)       # a log without a watch list
        # the tether's own
        assert raw(eng, "teth", n, state, prev, out, pvo, s_extremes=S_E, tether=t + 4, s_tether=S_T) == (E_ARG, -7)                      # misaligned
        assert raw(eng, "teth", n, state, prev, out, pvo, s_extremes=S_E, tether=t, s_tether=444) == (E_ARG, -7)              # below 7 * 64
        assert raw(eng, "teth", n, state, prev, out, pvo, s_extremes=S_E, tether=t, s_tether=450) == (E_ARG, -7)              # not a multiple of 4
        assert raw(eng, "teth", n, state, prev, out, pvo, s_extremes=S_E, tether=out.data_ptr(), s_tether=S_T) == (E_ARG, -7)             # aliases state_out
        assert "tether must not overlap" in last()
        assert raw(eng, "teth", n, state, prev, out, pvo, s_extremes=S_E, tether=pvo.data_ptr(), s_tether=S_T) == (E_ARG, -7)             # aliases prev_out
        assert "tether must not overlap" in last()
        assert raw(eng, "teth", n, state, prev, out, pvo, extremes=e, s_extremes=S_E, tether=e, s_tether=S_T) == (E_ARG, -7)              # aliases the extremes record
        assert "tether must not overlap" in last()
        # the mooring and the extremes are refused before the tether
        assert raw(eng, "teth", n, state, prev, out, pvo, mooring=m + 4, s_extremes=S_E, tether=t + 4, s_tether=S_T) == (E_ARG, -7)
        assert "tether" not in last()
        assert raw(eng, "teth", n, state, prev, out, pvo, extremes=e + 4, s_extremes=S_E, tether=t + 4, s_tether=S_T) == (E_ARG, -7)
        assert "tether" not in last()
        eng.set_watch([0, 320])
        assert raw(eng, "teth", n, state, prev, out, pvo, steps=5, log=log, s_extremes=S_E, tether=t, s_tether=S_T) == (E_ARG, -7)        # rows 0 .. 4 of 4
        assert raw(eng, "teth", n, state, prev, out, pvo, log=log, s_extremes=S_E, tether=log.data_ptr(), s_tether=S_T) == (E_ARG, -7)      # aliases the log
    # the probe
    lib, s = eng._lib, eng._stream(None)
    sp, wp, tp = state.data_ptr(), w.data_ptr(), w1.data_ptr()
    for args in ((n, None, S_IN, t, S_T, wp, S_W, tp, S_T1), (n, sp, S_IN, None, S_T, wp, S_W, tp, S_T1), (n, sp, S_IN, t, S_T, None, S_W, tp, S_T1),
                 (n, sp + 4, S_IN, t, S_T, wp, S_W, tp, S_T1), (n, sp, S_IN, t + 4, S_T, wp, S_W, tp, S_T1), (n, sp, S_IN, t, S_T, wp + 4, S_W, tp, S_T1),
                 (n, sp, S_IN, t, S_T, wp, S_W, tp + 4, S_T1),
                 (n, sp, 828, t, S_T, wp, S_W, tp, S_T1), (n, sp, S_IN, t, 444, wp, S_W, tp, S_T1), (n, sp, S_IN, t, S_T, wp, 380, tp, S_T1),
                 (n, sp, S_IN, t, S_T, wp, S_W, tp, 60),
                 (n + 1, sp, S_IN, t, S_T, wp, S_W, tp, S_T1), (-1, sp, S_IN, t, S_T, wp, S_W, tp, S_T1),
                 (n, sp, S_IN, t, S_T, sp, S_W, tp, S_T1), (n, sp, S_IN, t, S_T, t, S_W, tp, S_T1), (n, sp, S_IN, wp, S_T, wp, S_W, tp, S_T1),     # out overlaps an input
                 (n, sp, S_IN, t, S_T, wp, S_W, sp, S_T1), (n, sp, S_IN, t, S_T, wp, S_W, t, S_T1), (n, sp, S_IN, t, S_T, wp, S_W, wp, S_T1)):     # tension overlaps
        assert lib.hydro_tether_wrench(eng._h, *args, s) == E_ARG, args
    bare = type(eng)(n, DEV, RHO, G)                              # no parameters yet
    assert lib.hydro_tether_wrench(bare._h, n, sp, S_IN, t, S_T, wp, S_W, tp, S_T1, bare._stream(None)) == E_STATE
    bare.close()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all() and torch.isnan(w).all() and torch.isnan(w1).all()
    assert torch.isnan(e8).all()
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or overwritten - state_out,
    prev_out, log, the extremes record and the probe's two outputs - and the inputs are untouched."""
    st, pv = pop["st"], pop["pv"]
    n, tiles = 200, 4
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    rec = record_for(pop["rec"], n)
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m9, t7 = _guarded(pop["moor"][:n], S_M), _guarded(rec, S_T)
    empty = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32), (n, 1))
    e8 = _guarded(empty, S_E)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9, t7)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    w1 = torch.full((tiles * S_T1,), NAN, device=DEV)
    eng._check(eng._lib.hydro_tether_wrench(eng._h, n, state.data_ptr(), S_IN, t7.data_ptr(), S_T, w.data_ptr(), S_W, w1.data_ptr(), S_T1, eng._stream(None)))
    rc, written = raw(eng, "teth", n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, log=log, applied=a.data_ptr(), control=c17.data_ptr(),
                      mooring=m9.data_ptr(), extremes=e8.data_ptr(), s_extremes=S_E, tether=t7.data_ptr(), s_tether=S_T)
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    line, wrest = _unguard(w, n, 6, S_W)
    tension, trest = _unguard(w1, n, 1, S_T1)
    ext, erest = _unguard(e8, n, 8, S_E)
    assert all(np.isnan(r).all() for r in (rest, prest, wrest, trest, erest)), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9, t7), before))
    assert np.isfinite(line).all() and np.isfinite(tension).all(), "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want_ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
    want, want_prev = step(eng, "teth", cur, old, n, 3, step0=11, tether=_tiled(rec), extremes=want_ext, mooring=_tiled(pop["moor"][:n]),
                           control=_tiled(pop["ctl"][:n]), applied=_tiled(pop["applied"][:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint32), _from(want, n).view(np.uint32))
    assert np.array_equal(pv_out.view(np.uint32), _from(want_prev, n).view(np.uint32))
    assert np.array_equal(ext.view(np.uint32), _from(want_ext, n).view(np.uint32))
    W, T, _ = _probe(eng, st, rec, n)
    assert np.array_equal(line.view(np.uint32), W.view(np.uint32)) and np.array_equal(tension[:, 0].view(np.uint32), T.view(np.uint32))
    eng.close()


# ---- 7. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 322), consecutive bodies tied in pairs (2 i, 2 i + 1) but for every fifth pair: the line a tenth
    shorter than the distance between the two, the default constants for the pair."""
    sc = scenes.scene_c2(n=322)
    a = np.array([i for i in range(0, 322, 2) if (i // 2) % 5 != 4])
    pairs = np.stack([a, a + 1], axis=1)
    m = sc.params[:, 10].astype(np.float64)
    k, c = Tether.for_pair(m[a], m[a + 1], sc.dt)
    fa, fb = np.array([0.05, 0.0, -0.05]), np.array([0.0, 0.05, 0.05])
    d = np.linalg.norm(sc.state[a + 1, 0:3].astype(np.float64) + fb - sc.state[a, 0:3] - fa, axis=1)     # (unit quaternions at the start)
    return sc, dict(pairs=pairs, fairlead_a=fa, fairlead_b=fb, length=0.9 * d, stiffness=k, damping=c)


def test_sim_runners_agree_with_tethers_set(native_built):
    sc, lines = _scene()
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        buf = sim.set_tether(**lines)
        assert buf is sim.tether and tuple(buf.shape) == (6, 7, 64)
        go(sim)
        assert name != "graph" or sim._graph is not None
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc, implicit_drag=True)
    plain.run_resident(64)
    for name in ("resident", "chunks", "graph"):
        assert _same(finals["eager"], finals[name]), name
    free = plain.state()
    moved = np.linalg.norm(finals["eager"][:, 0:3] - free[:, 0:3], axis=1) > 1e-3
    tied = np.isin(np.arange(322), lines["pairs"].reshape(-1))
    assert moved[tied].mean() > 0.9 and not moved[~tied].any()                                           # the lines pulled, and only their own bodies
    plain.close()


def test_graph_replays_with_tethers_lines_bed_extremes_and_current_and_clear_tether(native_built):
    from silver2_isaacsim_amd.mooring import Mooring
    sc, lines = _scene()
    d = np.random.default_rng(5).normal(size=(321, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mk, mc = Mooring.for_body(sc.params[:321, 10].astype(np.float64), sc.dt)
    moorings = dict(anchor=sc.state[:321, 0:3].astype(np.float64) + 5.0 * d, fairlead=(0.05, 0.0, -0.05), length=4.9, stiffness=mk, damping=mc)
    bed, current = Seabed.for_step(-30.0, sc.dt), SeaState((0.4, -0.1, 0.0))
    g, r, never, cleared = (ClosedLoopSim(sc, implicit_drag=True) for _ in range(4))
    for s in (g, r, never):
        s.set_sea(current)
        s.set_seabed(bed)
        s.set_mooring(**moorings, bodies=np.arange(321))
        s.track_extremes()
    for s in (g, r):
        s.set_tether(**lines)
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state())
    assert _same(g.extremes.buffer.cpu().numpy(), r.extremes.buffer.cpu().numpy())
    never.run_resident(64)
    assert not np.array_equal(r.state(), never.state())
    # tension_max stays the mooring line's: its values are those of a mooring line's tension, on a trajectory the tether changed
    assert (r.extremes.tension_max() > 0).mean() > 0.5
    cleared.set_sea(current)
    cleared.set_seabed(bed)
    cleared.set_mooring(**moorings, bodies=np.arange(321))
    cleared.track_extremes()
    cleared.set_tether(**lines)
    cleared.clear_tether()
    assert cleared.tether is None
    cleared.run_resident(32)
    cleared.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state())
    waves = ClosedLoopSim(sc, implicit_drag=True)
    waves.set_tether(**lines)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_tether(**lines)
    for s in (g, r, never, cleared, waves, two_kernel):
        s.close()


# ---- 8. the hanging pair of tests/test_tether.py on the device ------------------------------------------------------------------------
def test_the_hanging_pairs_settle_with_the_submerged_weight_on_the_line_on_the_device(native_built):
    """64 copies of the buoy and its box, 128 bodies: tile 0 holds 32 pairs as neighbours (2 i, 2 i + 1), tile 1 holds 32 pairs
    with the buoys in lanes 0 .. 31 and their boxes in a permutation of lanes 32 .. 63.  Resident equals eager bit for bit."""
    st2, pv2, pr2, sc, dt, weight = hanging_pair()
    rng = np.random.default_rng(9)
    buoys = np.concatenate([np.arange(0, 64, 2), 64 + np.arange(32)])
    boxes = np.concatenate([np.arange(1, 64, 2), 96 + rng.permutation(32)])
    st, pv, pr = np.zeros((128, 13), np.float32), np.zeros((128, 6), np.float32), np.zeros((128, 11), np.float32)
    st[buoys], st[boxes], pv[buoys], pv[boxes], pr[buoys], pr[boxes] = st2[0], st2[1], pv2[0], pv2[1], pr2[0], pr2[1]
    spot = np.arange(64)
    for group in (buoys, boxes):
        st[group, 0], st[group, 1] = 20.0 * (spot % 8), 20.0 * (spot // 8)
    scene = scenes.Scene("hanging pairs", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g)
    k, c = Tether.for_pair(pr2[0, 10], pr2[1, 10], dt)
    lines = dict(pairs=np.stack([buoys, boxes], axis=1), length=LINE, stiffness=k, damping=c)
    sim, eager = ClosedLoopSim(scene, implicit_drag=True), ClosedLoopSim(scene, implicit_drag=True)
    for s in (sim, eager):
        s.set_tether(**lines)
    sim.run_resident(96, chunk=32)
    eager.run_eager(96)
    assert _same(sim.state(), eager.state())
    sim.run_resident(2400 - 96, chunk=64)
    s = sim.state().astype(np.float64)
    T = Tether(n=128, **lines).tension(s)
    speed = np.linalg.norm(s[:, 7:10], axis=1)
    print(f"[hanging pairs on the device] |v| <= {speed.max():.2e} m/s  T {T.min():.2f} .. {T.max():.2f} N  (m - rho V) g {weight:.2f} N  "
          f"buoys z {s[buoys, 2].min():+.5f} .. {s[buoys, 2].max():+.5f} m  boxes z {s[boxes, 2].min():+.5f} .. {s[boxes, 2].max():+.5f} m")
    assert speed.max() < 1e-5
    assert np.abs(T - weight).max() < 0.1
    assert np.abs((s[buoys, 2] - s[boxes, 2]) - (LINE + weight / k)).max() < 1e-3
    for x in (sim, eager):
        x.close()


def test_tethered_rov_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "tethered_rov.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    m = re.search(r"tether tension ([\d.]+) N", res.stdout)
    assert m and float(m.group(1)) > 0.0, res.stdout
    assert re.search(r"mooring tension ([\d.]+) N", res.stdout) and re.search(r"ROV depth ([\d.]+) m", res.stdout) and re.search(r"downstream ([-\d.]+) m", res.stdout)
