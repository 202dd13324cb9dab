"""Tether nets on the device (hydro_step_fused_tiled_multi_net): each layer of a net is an argument of the probe
hydro_tether_wrench, on its strided sub-record; without a net the entry is the extremes entry, with one layer the tether entry,
and trailing layers of zeros change no bit; the recorded wrench of a step is the host's fl(fl(fl(w + W_0) + W_1) + W_2) formed
from the extremes entry's recorded wrench and the probe's outputs; with implicit drag, applied wrench, pose hold, sea, bed and
mooring lines a step follows the fp64 step within the project's own bound; a launch of 7 steps equals 7 of 1 and (2, 5),
recorded rows included; the KE and NT instantiations; refusals and guard bands; ClosedLoopSim's three runners and a graph
replay; the hanging chain of tests/test_tether_net.py on the device; the example.

Sizes and population: n = 200, 321 and 322 and the four-layer net of tests/tether_net_population.py over the bodies of
tests/test_tether_gpu.py (layer 0 is its record); the mooring lines are those of tests/test_mooring.py.

Bounds: tether_reference.PROBE_BOUND (2 units of 2^-24 of the scale; each layer is section 22's evaluation) for the probe, and
integrator_oracle.STEP_ULP_BOUND (24) for the step, scales as in tests/test_tether_gpu.py with every layer's term magnitudes
added to the surrogate wrench.  Left out of comparisons with fp64: the sixteen bodies at layer 0's ties, as there."""
import ctypes
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
import tether_net_reference as tnr
import tether_reference as tr
from conftest import REPO
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from silver2_isaacsim_amd.tether import TetherNet
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, RHO, S_A,
                              S_C, S_IN, S_M, S_OUT, S_PV, S_PVO, _same, _same_bits, step, _tiled, _unguard, _untouched)
from tether_net_population import (check_net, hanging_chain, hanging_constants, HANG_SPEED, HANG_STEPS, HANG_TENSION, LAYER2_PAIR, LINK, net_for,
                                   net_population, OPEN_CHAIN, SIZES)
from tether_population import assert_antisymmetric, bodies_of
from tether_reference import PROBE_BOUND

pytestmark = pytest.mark.gpu
STEPS = (1, 7)
S_E = 8 * 64 + 36                                                 # the extremes record's tile stride in the guard tests


def S_N(layers):
    """The net's tile stride in the guard tests."""
    return 448 * layers + 44


@pytest.fixture(scope="module")
def pop(bed_pop, hold_pop):
    """The bodies of tests/test_tether_gpu.py (the 321 of tests/test_seabed_gpu.py and one more) with the net of
    tether_net_population.net_population and the mooring lines of mooring_population.line_population (body 321 has none)."""
    st, pv, params, applied, ctl = bed_pop
    more = hold_pop
    cat = lambda a, b: np.concatenate([a, b[321:322]])  # noqa: E731
    applied, ctl = cat(applied, more[3]), cat(ctl, more[4])
    params = {k: cat(params[k], more[2][k]) for k in params}
    st, pv, pr, net, groups = net_population()
    assert np.array_equal(pr, params["f32"])
    moor = np.concatenate([line_population(st[:321], params["f32"][:321]), np.zeros((1, 9), np.float32)])
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, net=net, groups=groups, moor=moor, ties=bodies_of(groups, "ties_0", "ties_c"))


def step_net(eng, cur, old, n, steps, *, net, layers, step0=0, applied=None, frame="world", control=None, mooring=None, extremes=None, implicit=False,
             ke=None, **kw):
    """resident_harness.step for the net entry: one launch through the engine; (state, prev_out)."""
    eng.step_fused_tiled_multi_net(cur, old, n, DT, steps, step0, net, layers, extremes, mooring, control, applied, frame, implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def raw_net(eng, n, state, prev, out, pvo, *, layers, s_tether, tether, steps=1, step0=0, implicit=0, log=None, fields=13, frame=0, applied=None,
            control=None, mooring=None, extremes=None):
    """resident_harness.raw for hydro_step_fused_tiled_multi_net: the guard tests' strides; (rc, rows_written from the sentinel -7)."""
    ptr = lambda b: b.data_ptr() if hasattr(b, "data_ptr") else b  # noqa: E731
    written = ctypes.c_int64(-7)
    rc = eng._lib.hydro_step_fused_tiled_multi_net(
        eng._h, n, ptr(state), S_IN, ptr(prev), S_PV, DT, steps, ptr(out), S_OUT, ptr(pvo), S_PVO,
        int(implicit), 1, None, ptr(log), 8, 4, fields, 1, 1, 0, ctypes.byref(written),
        ptr(applied), S_A, frame, ptr(control), S_C, ptr(mooring), S_M, ptr(extremes), S_E, ptr(tether), s_tether, layers, step0, eng._stream(None))
    return rc, written.value


def _same_bits_or_nan(a, b):
    """Bit for bit, but that a NaN equals a NaN whatever its payload: seven explicit steps carry a light, strongly damped body of
    the population out of the fp32 range (resident_harness._same_values), and which operand's payload a NaN inherits is the
    instruction's operand order - the compiler's choice, kernel by kernel.  Every number, every zero's sign and every
    infinity must agree exactly, and so must the places of the NaNs."""
    return bool(((a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32)
                  == b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _probes(eng, st, net, n, layers):
    """([W_l (n, 6)], [T_l (n,)]) of the per-layer probe on the net's sub-records."""
    w, t = eng.tether_net_wrench(_tiled(st[:n]), _tiled(net), n, layers)
    return [_from(x, n) for x in w], [_from(x, n)[:, 0] for x in t]


def test_population_is_what_it_was_designed_to_be(pop):
    check_net(pop["st"], pop["net"], pop["groups"])


# ---- 1. the probe, layer by layer, on the strided sub-records ---------------------------------------------------------------------------
def test_each_layer_is_an_argument_of_the_probe(pop, native_built):
    """hydro_tether_wrench on base + 448 l floats with the net's tile stride: the bits of the probe on the layer's own 7-field
    record; forces equal and opposite bit for bit per line; the fp64 reference within PROBE_BOUND, layer 0's ties aside."""
    st, ties = pop["st"], pop["ties"]
    worst = {"force": 0.0, "torque": 0.0, "tension": 0.0}
    for n in SIZES:
        eng = _engine(n, pop["params"]["f32"], "f32")
        net = net_for(pop["net"], n)
        W, T = _probes(eng, st, net, n, 4)
        off = ~np.isin(np.arange(n), ties)
        for l, rec in enumerate(tnr.layers_of(net)):
            assert np.isfinite(W[l]).all() and np.isfinite(T[l]).all()
            pulled = assert_antisymmetric(W[l], T[l], rec)
            assert pulled >= (n // 4, n // 4, 2, 0)[l] and (l < 3 or not W[l].any())
            alone = _from(eng.tether_wrench(_tiled(st[:n]), _tiled(rec), n), n)
            assert _same(alone, W[l]), (n, l)
            s = st[:n]
            on = tr.taut(rec, s)
            ref, scale, ref_T, scale_T = tr.wrench(rec, s, on), tr.wrench_scales(rec, s, on), tr.tension(rec, s, on), tr.tension_scale(rec, s, on)
            keep = off if l == 0 else np.ones(n, bool)
            live = (ref_T > 0) & keep
            idle = ~live & keep
            assert not W[l][idle].any() and not np.signbit(W[l][idle]).any() and not T[l][idle].any()
            if not live.any():
                continue
            assert (T[l][live] > 0).all()
            err = np.abs(W[l][live] - ref[live]) / (tr.ULP * scale[live])
            worst["force"] = max(worst["force"], float(err[:, 0:3].max()))
            worst["torque"] = max(worst["torque"], float(err[:, 3:6].max()))
            worst["tension"] = max(worst["tension"], float((np.abs(T[l][live] - ref_T[live]) / (tr.ULP * scale_T[live])).max()))
        eng.close()
    print("[tether net, per-layer probe] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {PROBE_BOUND:g})")
    assert max(worst.values()) <= PROBE_BOUND, worst


# ---- 2. no net, one layer, trailing layers of zeros ----------------------------------------------------------------------------------------
OPTIONS = ("log", "applied", "control", "sea", "bed", "mooring", "extremes")


@COEFFS
@DRAG
def test_no_net_one_layer_and_trailing_zero_layers(coeff, implicit, pop, native_built):
    """Bit for bit - state, prev_out, kinetic energy, the recorded state and wrench and the extremes record - with none of log,
    applied wrench, control, sea, bed, mooring lines and extremes, with each of them alone, and with all of them:
      tether = NULL (layers = 1 and an ignored 9)        = hydro_step_fused_tiled_multi_ext
      layers = 1                                       = hydro_step_fused_tiled_multi_teth with the same record (a NaN of the seven
                                                         explicit steps may carry another payload: _same_bits_or_nan)
      [layer 0 | zeros | zeros], 3 layers              = layers = 1
      the designed net, 4 layers (layer 3 is zeros)    = its first 3 layers."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        watched = sorted({b for b in (0, 5, 8, 11, 40, 63, 64, 80, 130, n - 1) if b < n})
        eng.set_watch(watched)
        a, c17, m9 = _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n]), _tiled(pop["moor"][:n])
        net4 = net_for(pop["net"], n)
        rec0, zeros = net4[:, 0:7], net4[:, 21:28]
        assert not zeros[:, 0:6].any()
        one, padded, three, four = _tiled(rec0), _tiled(np.concatenate([rec0, zeros, zeros], axis=1)), _tiled(net4[:, 0:21]), _tiled(net4)
        for chosen in [()] + [(o,) for o in OPTIONS] + [OPTIONS]:
            eng.set_sea(SEA if "sea" in chosen else None)
            eng.set_seabed(BED if "bed" in chosen else None)
            for steps in STEPS:
                def run(launch):
                    cur, old = _buffers(st, pv, n)
                    ke = _ke()
                    kw = dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if "log" in chosen else {}
                    ext = eng.extremes_reset(eng.alloc_tiled(8, n), n) if "extremes" in chosen else None
                    state, prev = launch(cur, old, extremes=ext, mooring=m9 if "mooring" in chosen else None, control=c17 if "control" in chosen else None,
                                         applied=a if "applied" in chosen else None, implicit=implicit, ke=ke, **kw)
                    torch.cuda.synchronize()
                    return [state, prev, ke] + ([kw["log"]] if kw else []) + ([ext] if ext is not None else [])
                old_entry = lambda entry, tether: lambda cur, old, **kw: step(eng, entry, cur, old, n, steps, step0=3, tether=tether, **kw)  # noqa: E731
                net_entry = lambda net, layers: lambda cur, old, **kw: step_net(eng, cur, old, n, steps, step0=3, net=net, layers=layers, **kw)  # noqa: E731
                same = lambda x, y: all(_same_bits(p, q) for p, q in zip(x, y))  # noqa: E731
                want = run(old_entry("ext", None))
                assert same(run(net_entry(None, 1)), want) and same(run(net_entry(None, 9)), want), (n, steps, chosen)
                want = run(old_entry("teth", one))                # (another kernel: _same_bits_or_nan)
                alike = lambda x, y: all(_same_bits_or_nan(p, q) for p, q in zip(x, y))  # noqa: E731
                assert alike(run(net_entry(one, 1)), want), (n, steps, chosen)
                assert alike(run(net_entry(padded, 3)), want), (n, steps, chosen)
                assert steps == 7 and not implicit or same(run(net_entry(one, 1)), want), (n, steps, chosen)     # no NaN: the very bits
                assert same(run(net_entry(four, 4)), run(net_entry(three, 3))), (n, steps, chosen)
        eng.close()


# ---- 3. the order of the additions -------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
def test_the_recorded_wrench_is_the_hosts_sum_in_ascending_layer_order(coeff, semantics, implicit, pop, native_built):
    """One step over the bed, through the sea, with the mooring lines, every body watched with its wrench.  The logged wrench
    equals, bit for bit, fl(fl(fl(w + W_0) + W_1) + W_2) in fp32 on the host: w the extremes entry's logged wrench, W_l the
    probe's output for layer l, a layer that does not pull skipped (no +0 is added).  A body pulled in at most one layer has the
    state of the tether entry's step with that layer alone."""
    st, pv = pop["st"], pop["pv"]
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(sea)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        net = net_for(pop["net"], n)
        m9 = _tiled(pop["moor"][:n])
        W, T = _probes(eng, st, net, n, 4)
        pulls = np.stack([t > 0 for t in T])
        count = pulls.sum(axis=0)
        assert (count == 0).sum() >= n // 8 and (count == 1).sum() >= n // 4 and (count == 2).sum() >= 14 and (count == 3).sum() >= 1 and not pulls[3].any()

        def one(launch):
            log = torch.full((1, 19, n), NAN, dtype=torch.float32, device=DEV)
            cur, old = _buffers(st, pv, n)
            state, _ = launch(cur, old, mooring=m9, implicit=implicit, log=log)
            torch.cuda.synchronize()
            return _from(state, n), log[0].cpu().numpy().T                                       # (n, 13), (n, 19)
        got_state, got_log = one(lambda cur, old, **kw: step_net(eng, cur, old, n, 1, step0=7, net=_tiled(net), layers=4, **kw))
        ext_state, ext_log = one(lambda cur, old, **kw: step(eng, "ext", cur, old, n, 1, step0=7, **kw))
        total = ext_log[:, 13:19].copy()
        for l in range(3):
            total = np.where(pulls[l][:, None], total + W[l], total)
        assert total.dtype == np.float32 and _same(np.ascontiguousarray(got_log[:, 13:19]), np.ascontiguousarray(total)), n
        assert _same(np.ascontiguousarray(got_log[:, 0:13]), got_state)
        assert _same(got_state[count == 0], ext_state[count == 0])
        for l in range(3):
            rec = np.ascontiguousarray(net[:, 7 * l:7 * l + 7])
            alone_state, alone_log = one(lambda cur, old, **kw: step(eng, "teth", cur, old, n, 1, step0=7, tether=_tiled(rec), **kw))
            only = pulls[l] & (count == 1)
            assert only.sum() >= (8, 8, 0)[l]
            assert _same(got_state[only], alone_state[only]) and _same(np.ascontiguousarray(got_log[only]), np.ascontiguousarray(alone_log[only])), (n, l)
        eng.close()


# ---- 4. everything together against fp64 ---------------------------------------------------------------------------------------------
@COEFFS
def test_one_step_with_everything_against_fp64(coeff, pop, native_built):
    """Implicit drag + applied wrench + pose hold + sea with two waves + bed + mooring lines + the net.  Reference as in
    tests/test_tether_gpu.py, the tethers' term the fp64 sum over the layers; left out: bodies within 1e-4 of a branch of the
    hydrodynamic model, and the ties with a damper of the mooring lines and of layer 0."""
    from mooring_population import TIES as MOOR_TIES
    st, pv, applied, ctl = pop["st"], pop["pv"], pop["applied"], pop["ctl"]
    pr = pop["params"][coeff]
    worst = {}
    sea = SeaState(SEA.current).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])
    assert len(sea.waves) == 2
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(sea)
        eng.set_seabed(BED)
        net, moor = net_for(pop["net"], n), pop["moor"][:n]
        w = _from(eng.sea_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        keep[MOOR_TIES[4:]] = False
        keep[bodies_of(pop["groups"], "ties_c")] = False
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step_net(eng, cur, old, n, 1, step0=7, net=_tiled(net), layers=4, mooring=_tiled(moor), control=_tiled(ctl[:n]), applied=_tiled(applied[:n]),
                          implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        on_m = mr.taut_fp32(moor, st[:n])
        on_t = [tr.taut_fp32(rec, st[:n]) for rec in tnr.layers_of(net)]
        extra = br.wrench(BED, st[:n], pr[:n], touch) + mr.wrench(moor, st[:n], on_m) + tnr.wrench(net, st[:n], on_t)
        extra_scale = br.wrench_scales(BED, st[:n], pr[:n], touch) + mr.wrench_scales(moor, st[:n], on_m) + tnr.wrench_scales(net, st[:n], on_t)
        both = (tr.tension(net[:, 0:7], st[:n], on_t[0]) > 0) & (tr.tension(net[:, 7:14], st[:n], on_t[1]) > 0)
        assert (both & keep).sum() >= 8
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=extra[keep],
                                    bed_scale=extra_scale[keep])
        eng.close()
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[sea + applied + pose hold + bed + lines + net of 4 layers, implicit, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g})")
    assert max(per_group.values()) <= B, worst


# ---- 5. step counts and the recorder -----------------------------------------------------------------------------------------------------
def _watched_chain(pop, n):
    """The ring of tile 0 (both neighbours of every body of it), the two ends and the interior of the open chain, layer 2's pair,
    bodies of tile 2, and the last body."""
    return sorted({int(b) for b in list(pop["groups"]["ring"]) + list(OPEN_CHAIN) + list(LAYER2_PAIR) + [128, 159, 160, 191, n - 2, n - 1] if b < n})


@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    """7 steps = 7 x 1 = (2, 5) with step0 advanced: state, prev_out and every recorded row (state and wrench) of the watched
    bodies - both ends and the interior bodies of the chains."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        watched = _watched_chain(pop, n)
        eng.set_watch(watched)
        net = net_for(pop["net"], n)
        assert (tnr.pulls(net, st[:n])[:, watched].sum(axis=0) >= 2).sum() >= 16
        lines, m9 = _tiled(net), _tiled(pop["moor"][:n])

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                step_net(eng, cur, old, n, k, step0=100 + done, net=lines, layers=4, mooring=m9, implicit=implicit, log=log, every=1, phase=1, row0=done)
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
    """KE = true (the state bits of the launch without sampling, and with implicit drag the energy pair of the returned state
    against scenes.kinetic_energy_fp64 to 1e-12, with and without the rotational term) and NT = true (set_tuning(0, 0, 1): the
    bits of the temporal launch), with sea, bed, pose hold, applied wrench, mooring lines and extremes active."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        lines, m9, a, c17 = _tiled(net_for(pop["net"], n)), _tiled(pop["moor"][:n]), _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n])

        def run(ke=None, **kw):
            cur, old = _buffers(st, pv, n)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            state, prev = step_net(eng, cur, old, n, 7, step0=5, net=lines, layers=4, extremes=ext, mooring=m9, control=c17, applied=a, implicit=implicit, ke=ke, **kw)
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
    """The tether entry's refusals, then: layers outside 1 .. 4, a stride below 448 L, the net's last layer over an output."""
    n, L = 322, 3
    tiles, s_n = (n + 63) // 64, S_N(3)
    st, pv = pop["st"], pop["pv"]
    eng = _engine(n, pop["params"]["f32"], "f32")
    state, prev = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV)
    m9, net = _guarded(pop["moor"][:n], S_M), _guarded(net_for(pop["net"], n, 3), s_n)
    # one allocation: the net's copy at its head, and room behind it for an output that starts inside the last layer of its last tile
    inside = (tiles - 1) * s_n + 448 * (L - 1) + 64
    arena = torch.full((inside + tiles * S_OUT,), NAN, device=DEV)
    arena[:tiles * s_n] = net
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG = -1
    t, e = net.data_ptr(), e8.data_ptr()
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    call = lambda **kw: raw_net(eng, n, state, prev, kw.pop("out", out), pvo, **{**dict(layers=L, s_tether=s_n, tether=t), **kw})  # noqa: E731
    for bed, sea in ((BED, None), (BED, SEA), (None, None)):
        eng.set_seabed(bed)
        eng.set_sea(sea)
        # the tether entry's, with a net and without
        for lines in (t, None):
            assert call(tether=lines, step0=-1) == (E_ARG, -7)
            assert call(tether=lines, steps=0) == (E_ARG, -7)
            assert call(tether=lines, mooring=m9.data_ptr() + 4) == (E_ARG, -7)
            assert call(tether=lines, extremes=e + 4) == (E_ARG, -7)
            assert call(tether=lines, extremes=state.data_ptr()) == (E_ARG, -7)
        assert call(tether=t + 4) == (E_ARG, -7)                                                   # misaligned
        assert call(tether=out.data_ptr()) == (E_ARG, -7) and "tether must not overlap" in last()    # aliases state_out
        # the net's own
        for layers in (0, 5, -1):
            assert call(layers=layers) == (E_ARG, -7) and "tether_layers" in last(), layers
        assert call(layers=0, mooring=m9.data_ptr() + 4) == (E_ARG, -7) and "tether_layers" not in last()     # the mooring is refused first
        assert raw_net(eng, n, state, prev, out, pvo, layers=5, tether=None, s_tether=0)[0] == 0         # without a net the layers are not looked at
        assert call(s_tether=448 * L - 64) == (E_ARG, -7) and "stride" in last()
        assert call(layers=4) == (E_ARG, -7) and "stride" in last()                                 # the stride of three layers is below 448 * 4
        assert call(layers=2)[0] == 0                                                              # (and is any stride for two)
        # the LAST layer of the last tile over state_out and over the extremes record
        head = arena.data_ptr()
        assert call(tether=head, out=head + 4 * inside) == (E_ARG, -7) and "tether must not overlap" in last()
        assert call(tether=head, extremes=head + 4 * inside) == (E_ARG, -7) and "tether must not overlap" in last()
        assert call(tether=head + 4 * 64, extremes=head, layers=1, s_tether=s_n) == (E_ARG, -7)
    torch.cuda.synchronize()
    out[:] = NAN                                                   # (the accepted launches above wrote state_out and prev_out)
    pvo[:] = NAN
    for layers in (0, 5, -1):
        assert call(layers=layers, log=None) == (E_ARG, -7)
    assert call(s_tether=448 * L - 64) == (E_ARG, -7)
    assert call(tether=arena.data_ptr(), extremes=arena.data_ptr() + 4 * inside) == (E_ARG, -7)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all() and torch.isnan(e8).all()
    assert torch.isnan(arena[tiles * s_n:]).all() and _untouched(arena[:tiles * s_n], net.cpu().numpy())
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer - the net's padding behind its last layer included: the bodies' outputs are those of the tightly packed
    launch, no sentinel is read or overwritten, and the inputs are untouched."""
    st, pv = pop["st"], pop["pv"]
    n, tiles, L = 200, 4, 3
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    rec = net_for(pop["net"], n, L)
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m9, t21 = _guarded(pop["moor"][:n], S_M), _guarded(rec, S_N(L))
    empty = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32), (n, 1))
    e8 = _guarded(empty, S_E)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9, t21)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    rc, written = raw_net(eng, n, state, prev, out, pvo, layers=L, s_tether=S_N(L), tether=t21.data_ptr(), steps=3, step0=11, implicit=implicit, log=log,
                          applied=a.data_ptr(), control=c17.data_ptr(), mooring=m9.data_ptr(), extremes=e8.data_ptr())
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    ext, erest = _unguard(e8, n, 8, S_E)
    assert all(np.isnan(r).all() for r in (rest, prest, erest)), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9, t21), before))
    assert np.isfinite(got).all() or not implicit, "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want_ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
    want, want_prev = step_net(eng, cur, old, n, 3, step0=11, net=_tiled(rec), layers=L, extremes=want_ext, mooring=_tiled(pop["moor"][:n]),
                               control=_tiled(pop["ctl"][:n]), applied=_tiled(pop["applied"][:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert _same(got, _from(want, n)) and _same(pv_out, _from(want_prev, n)) and _same(ext, _from(want_ext, n))
    eng.close()


# ---- 7. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 322): in every tile chains of five consecutive bodies (5 j .. 5 j + 4 of the tile, but for every
    fourth chain), each link a tenth shorter than the distance between its two fairleads, uniform constants from for_chain per
    chain; plus a bridle on the first link of every chain of tile 0."""
    sc = scenes.scene_c2(n=322)
    m = sc.params[:, 10].astype(np.float64)
    fa, fb = np.array([0.05, 0.0, -0.05]), np.array([0.0, 0.05, 0.05])
    links, k, c = [], [], []
    for t in range(6):
        for j in range(12):
            bodies = 64 * t + 5 * j + np.arange(5)
            if j % 4 == 3 or bodies[-1] >= 322:
                continue
            kj, cj = TetherNet.for_chain(m[bodies], sc.dt)
            for a, b in zip(bodies[:-1], bodies[1:]):
                links.append((a, b))
                k.append(0.5 * kj)                                # (half: the bridle doubles the first link of a chain of tile 0)
                c.append(0.5 * cj)
            if t == 0:
                links.append((bodies[0], bodies[1]))
                k.append(0.5 * kj)
                c.append(0.5 * cj)
    links = np.array(links)
    d = np.linalg.norm(sc.state[links[:, 1], 0:3].astype(np.float64) + fb - sc.state[links[:, 0], 0:3] - fa, axis=1)     # (unit quaternions at the start)
    return sc, dict(links=links, fairlead_a=fa, fairlead_b=fb, length=0.9 * d, stiffness=np.array(k), damping=np.array(c))


def test_sim_runners_agree_with_a_net_set(native_built):
    sc, net = _scene()
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        buf = sim.set_tether_net(**net)
        assert buf is sim.tether_net and sim.tether_layers == 3 and tuple(buf.shape) == (6, 21, 64)
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
    tied = np.isin(np.arange(322), net["links"].reshape(-1))
    assert moved[tied].mean() > 0.9 and not moved[~tied].any()                                           # the lines pulled, and only their own bodies
    plain.close()


def test_graph_replays_with_a_net_lines_bed_extremes_and_current_and_clear_tether_net(native_built):
    from silver2_isaacsim_amd.mooring import Mooring
    sc, net = _scene()
    d = np.random.default_rng(5).normal(size=(321, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mk, mc = Mooring.for_body(sc.params[:321, 10].astype(np.float64), sc.dt)
    moorings = dict(anchor=sc.state[:321, 0:3].astype(np.float64) + 5.0 * d, fairlead=(0.05, 0.0, -0.05), length=4.9, stiffness=mk, damping=mc)
    bed, current = Seabed.for_step(-30.0, sc.dt), SeaState((0.4, -0.1, 0.0))
    g, r, never, cleared = (ClosedLoopSim(sc, implicit_drag=True) for _ in range(4))
    for s in (g, r, never, cleared):
        s.set_sea(current)
        s.set_seabed(bed)
        s.set_mooring(**moorings, bodies=np.arange(321))
        s.track_extremes()
    for s in (g, r):
        s.set_tether_net(**net)
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state())
    assert _same(g.extremes.buffer.cpu().numpy(), r.extremes.buffer.cpu().numpy())
    never.run_resident(64)
    assert not np.array_equal(r.state(), never.state())
    assert (r.extremes.tension_max() > 0).mean() > 0.5          # tension_max stays the mooring line's
    cleared.set_tether_net(**net)
    cleared.clear_tether_net()
    assert cleared.tether_net is None and cleared.tether_layers == 0
    cleared.run_resident(32)
    cleared.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state())
    with pytest.raises(ValueError, match=r"clear_tether_net\(\) first"):
        r.set_tether(pairs=[[0, 1]], length=1.0, stiffness=1.0)
    waves = ClosedLoopSim(sc, implicit_drag=True)
    waves.set_tether_net(**net)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_tether_net(**net)
    for s in (g, r, never, cleared, waves, two_kernel):
        s.close()


# ---- 8. the hanging chain of tests/test_tether_net.py on the device -----------------------------------------------------------------
def test_the_hanging_chains_carry_the_submerged_weight_below_each_link_on_the_device(native_built):
    """64 copies of the buoy and its four boxes, 340 bodies (the last tile has 20 live lanes): twelve chains to a tile, in even
    tiles and in the last as consecutive bodies, in the other odd tiles with the buoys in lanes 0 .. 11 and the boxes in a permutation of lanes 12 .. 59;
    lanes 60 .. 63 hold buoys without a line.  Resident equals eager bit for bit; after HANG_STEPS steps the thresholds of
    tests/test_tether_net.py hold for every copy."""
    st5, pv5, pr5, sc, dt, hang = hanging_chain()
    rng = np.random.default_rng(9)
    n = 340
    chains = []
    for t in range(6):
        lanes = np.arange(60).reshape(12, 5) if t % 2 == 0 or t == 5 else np.concatenate([np.arange(12)[:, None], 12 + rng.permutation(48).reshape(12, 4)], axis=1)
        chains += [64 * t + row for row in lanes[:4 if t == 5 else 12]]
    chains = np.array(chains)
    assert chains.shape == (64, 5) and chains.max() < n and len(np.unique(chains)) == 320
    st, pv, pr = np.tile(st5[0], (n, 1)), np.tile(pv5[0], (n, 1)), np.tile(pr5[0], (n, 1))          # (spare lanes: buoys)
    for i in range(5):
        st[chains[:, i]], pv[chains[:, i]], pr[chains[:, i]] = st5[i], pv5[i], pr5[i]
    spot = np.arange(n)
    st[:, 0], st[:, 1] = 20.0 * (spot % 20), 20.0 * (spot // 20)
    for i in range(1, 5):
        st[chains[:, i], 0:2] = st[chains[:, 0], 0:2]
    scene = scenes.Scene("hanging chains", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g)
    k, c = hanging_constants(pr5, dt)
    links = np.concatenate([np.stack([chains[:, i], chains[:, i + 1]], axis=1) for i in range(4)])
    lines = dict(links=links, length=LINK, stiffness=k, damping=c, layer=np.repeat([0, 1, 0, 1], 64))
    sim, eager = ClosedLoopSim(scene, implicit_drag=True), ClosedLoopSim(scene, implicit_drag=True)
    for s in (sim, eager):
        s.set_tether_net(**lines)
        assert s.tether_layers == 2
    sim.run_resident(96, chunk=32)
    eager.run_eager(96)
    assert _same(sim.state(), eager.state())
    sim.run_resident(HANG_STEPS - 96, chunk=64)
    s = sim.state().astype(np.float64)
    T = TetherNet(n=n, **lines).tensions(s).reshape(4, 64)
    speed = np.linalg.norm(s[:, 7:10], axis=1)
    off = np.abs(T - hang[:, None])
    print(f"[hanging chains on the device] |v| <= {speed.max():.3e} m/s (threshold {HANG_SPEED:g})  T " + "  ".join(f"{a:.2f} .. {b:.2f}" for a, b in zip(T.min(axis=1), T.max(axis=1)))
          + " N  weight below " + " ".join(f"{w:.2f}" for w in hang) + f" N  |T - weight| <= {off.max():.4f} N (threshold {HANG_TENSION:g})")
    assert speed.max() < HANG_SPEED
    assert off.max() < HANG_TENSION
    for x in (sim, eager):
        x.close()


def test_umbilical_cable_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "umbilical_cable.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    tensions = re.search(r"link tensions \(N\):((?: +[\d.]+)+)", res.stdout)
    assert tensions and max(float(x) for x in tensions.group(1).split()) > 0.0, res.stdout
    assert re.search(r"ROV depth ([\d.]+) m", res.stdout) and re.search(r"sag ([-\d.]+) m", res.stdout)
