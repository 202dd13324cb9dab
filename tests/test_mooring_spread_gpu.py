"""Mooring spreads on the device (hydro_step_fused_tiled_multi_spread): each layer of a spread is an argument of the probe
hydro_mooring_wrench, on its strided sub-record; without a spread the entry is the link-tension entry, with one layer that entry
with the same record, and trailing layers of zeros change no bit; the recorded wrench of a step is the host's
fl(fl(fl(w + W_0) + W_1) + W_2) formed from the recorded wrench of the step without lines and the probe's outputs, also with a
two-layer tether net behind the spread; tension_max of the extremes record is the largest tension of a body's lines, folded over
layers and steps; with implicit drag, applied wrench, pose hold, sea, bed, a four-layer spread and a two-layer net a step follows
the fp64 step within the project's own bound; a launch of 7 steps equals 7 of 1 and (2, 5), recorded rows included; the KE and NT
instantiations; one row of the resident ladder; refusals and guard bands; malformed layers; ClosedLoopSim's three runners and a
graph replay; the two physical cases of tests/test_mooring_spread.py on the device; the example.

Sizes and population: n = 200 and 321 and the four-layer spread of tests/mooring_spread_population.py built over the bodies of
tests/test_tether_net_gpu.py (layer 0 is mooring_population.line_population of them); the tether net is that module's.

Bounds: mooring_reference.PROBE_BOUND (2 units of 2^-24 of the scale; each layer is section 19's evaluation - the same function,
so the bound is not derived again) for the probe, and integrator_oracle.STEP_ULP_BOUND (24) for the step, scales as in
tests/test_tether_net_gpu.py with every layer's term magnitudes added to the surrogate wrench.  Left out of comparisons with
fp64: the bodies at layer 0's ties, as in tests/test_mooring_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mooring_reference as mr
import mooring_spread_reference as msr
import seabed_reference as br
import sea_reference as sr
import tether_net_reference as tnr
import tether_reference as tr
from conftest import REPO
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.mooring import Mooring, MooringSpread
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import buoy, DEPTH, line_population, OFF_TIES, population_report, TIES
from mooring_reference import PROBE_BOUND
from mooring_spread_population import check_spread, SIZES, spread_population
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, ENTRIES, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, RHO,
                              S_A, S_C, S_IN, S_OUT, S_PV, S_PVO, _same, _same_bits, step, _tiled, _unguard, _untouched)
from tether_net_population import net_for, net_population
from tether_population import bodies_of

pytestmark = pytest.mark.gpu
STEPS = (1, 7)
S_E = 8 * 64 + 36                                                 # the extremes record's tile stride in the guard tests
S_T2 = 448 * 2 + 44                                               # a two-layer net's
S_P2 = 64 * 2 + 20                                                # its link tensions'


def S_SP(layers):
    """The spread's tile stride in the guard tests."""
    return 576 * layers + 52


@pytest.fixture(scope="module")
def pop(bed_pop):
    """The first 321 bodies of tests/test_tether_net_gpu.py (those of tests/test_mooring_gpu.py but for one body the net moved) with the
    designed spread built over them, and the tether net of tests/tether_net_population.py."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, groups = net_population()
    assert np.array_equal(pr[:321], params["f32"])
    st, pv = st[:321], pv[:321]
    spread = spread_population(st, params["f32"], line_population(st, params["f32"]))
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, spread=spread, net=net, groups=groups)


def step_spread(eng, cur, old, n, steps, *, spread, layers, step0=0, tether=None, net_layers=1, peaks=None, extremes=None, applied=None, frame="world",
                control=None, implicit=False, ke=None, **kw):
    """resident_harness.step for the spread entry: one launch through the engine; (state, prev_out)."""
    eng.step_fused_tiled_multi_spread(cur, old, n, DT, steps, step0, spread, layers, tether, net_layers, peaks, extremes, control, applied, frame,
                                      implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def raw_spread(eng, n, state, prev, out, pvo, *, layers, s_mooring, mooring, steps=1, step0=0, implicit=0, log=None, fields=13, frame=0, applied=None,
               control=None, extremes=None, tether=None, net_layers=2, peaks=None):
    """resident_harness.raw for hydro_step_fused_tiled_multi_spread: the guard tests' strides; (rc, rows_written from the sentinel -7)."""
    ptr = lambda b: b.data_ptr() if hasattr(b, "data_ptr") else b  # noqa: E731
    written = ctypes.c_int64(-7)
    rc = eng._lib.hydro_step_fused_tiled_multi_spread(
        eng._h, n, ptr(state), S_IN, ptr(prev), S_PV, DT, steps, ptr(out), S_OUT, ptr(pvo), S_PVO,
        int(implicit), 1, None, ptr(log), 8, 4, fields, 1, 1, 0, ctypes.byref(written),
        ptr(applied), S_A, frame, ptr(control), S_C, ptr(mooring), s_mooring, layers, ptr(extremes), S_E, ptr(tether), S_T2, net_layers,
        ptr(peaks), S_P2, step0, eng._stream(None))
    return rc, written.value


def _same_bits_or_nan(a, b):
    """Bit for bit, but that a NaN equals a NaN whatever its sign and payload: seven explicit steps carry a light, strongly damped
    body of the population out of the fp32 range, and which operand's bits a NaN inherits is the instruction's operand order - the
    compiler's choice, kernel by kernel.  Every number, every zero's sign and every infinity must agree
    exactly, and so must the places of the NaNs."""
    return bool(((a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32)
                  == b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _probes(eng, st, spread, n, layers):
    """[W_l (n, 6)] of the per-layer probe on the spread's sub-records."""
    return [_from(x, n) for x in eng.mooring_spread_wrench(_tiled(st[:n]), _tiled(spread), n, layers)]


def _tensions_by_ext(eng, st, pv, spread, n, layers, implicit=False):
    """[T_l (n,)]: tension_max that ONE step of the extremes entry leaves in an empty record with layer l alone as its mooring record."""
    out = []
    for rec in msr.layers_of(spread)[:layers]:
        cur, old = _buffers(st, pv, n)
        ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
        step(eng, "ext", cur, old, n, 1, extremes=ext, mooring=_tiled(np.ascontiguousarray(rec)), implicit=implicit)
        torch.cuda.synchronize()
        out.append(_from(ext, n)[:, 7])
    return out


def test_population_is_what_it_was_designed_to_be(pop):
    for n in SIZES:
        check_spread(pop["st"], pop["spread"], n)


# ---- 1. the probe, layer by layer, on the strided sub-records ---------------------------------------------------------------------------
def test_each_layer_is_an_argument_of_the_probe(pop, native_built):
    """hydro_mooring_wrench on base + 576 l floats with the spread's tile stride: the bits of the probe on the layer's own 9-field
    record; the fp64 reference within PROBE_BOUND, layer 0's ties aside."""
    st = pop["st"]
    worst = {"force": 0.0, "torque": 0.0}
    for n in SIZES:
        eng = _engine(n, pop["params"]["f32"], "f32")
        spread = pop["spread"][:n]
        W = _probes(eng, st, spread, n, 4)
        off = ~np.isin(np.arange(n), TIES)
        for l, rec in enumerate(msr.layers_of(spread)):
            rec = np.ascontiguousarray(rec)
            assert np.isfinite(W[l]).all()
            alone = _from(eng.mooring_wrench(_tiled(st[:n]), _tiled(rec), n), n)
            assert _same(alone, W[l]), (n, l)
            s = st[:n]
            on = mr.taut_fp32(rec, s)
            ref, scale = mr.wrench(rec, s, on), mr.wrench_scales(rec, s, on)
            keep = off if l == 0 else np.ones(n, bool)
            live = (mr.tension(rec, s, on) > 0) & keep
            idle = ~live & keep
            assert not W[l][idle].any() and not np.signbit(W[l][idle]).any()
            assert live.sum() >= (32, 32, 8, 0)[l] and (l < 3 or not W[l].any())
            if not live.any():
                continue
            err = np.abs(W[l][live] - ref[live]) / (mr.ULP * scale[live])
            worst["force"] = max(worst["force"], float(err[:, 0:3].max()))
            worst["torque"] = max(worst["torque"], float(err[:, 3:6].max()))
        eng.close()
    print("[mooring spread, per-layer probe] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {PROBE_BOUND:g})")
    assert max(worst.values()) <= PROBE_BOUND, worst


# ---- 2. no spread, one layer, trailing layers of zeros ----------------------------------------------------------------------------------
OPTIONS = ("log", "applied", "control", "sea", "bed", "extremes", "net", "peaks")


@COEFFS
@DRAG
def test_no_spread_one_layer_and_trailing_zero_layers(coeff, implicit, pop, native_built):
    """Bit for bit - state, prev_out, kinetic energy, the recorded state and wrench, the extremes record and the link tensions -
    with none of log, applied wrench, control, sea, bed, extremes, a two-layer net and its link tensions, with each of them alone
    (the link tensions with their net), and with all of them:
      mooring = NULL (layers = 1 and an ignored 9)     = hydro_step_fused_tiled_multi_peak
      layers = 1                                       = hydro_step_fused_tiled_multi_peak with the same record (a NaN of the seven
                                                         explicit steps may carry another sign or payload: _same_bits_or_nan)
      [layer 0 | zeros | zeros], 3 layers              = layers = 1
      the designed spread, 4 layers (layer 3 is zeros) = its first 3 layers."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        watched = sorted({b for b in (0, 5, 8, 11, 40, 63, 64, 72, 73, 80, 130, n - 1) if b < n})
        eng.set_watch(watched)
        a, c17, net2 = _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n]), _tiled(net_for(pop["net"], n, 2))
        sp4 = pop["spread"][:n]
        rec0, zeros = sp4[:, 0:9], sp4[:, 27:36]
        assert not zeros.any()
        one, padded, three, four = _tiled(rec0), _tiled(np.concatenate([rec0, zeros, zeros], axis=1)), _tiled(sp4[:, 0:27]), _tiled(sp4)
        for chosen in [()] + [(o,) for o in OPTIONS[:-1]] + [("net", "peaks")] + [OPTIONS]:
            eng.set_sea(SEA if "sea" in chosen else None)
            eng.set_seabed(BED if "bed" in chosen else None)
            for steps in STEPS:
                def run(launch):
                    cur, old = _buffers(st, pv, n)
                    ke = _ke()
                    kw = dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if "log" in chosen else {}
                    ext = eng.extremes_reset(eng.alloc_tiled(8, n), n) if "extremes" in chosen else None
                    peaks = eng.alloc_tiled(2, n) if "peaks" in chosen else None
                    state, prev = launch(cur, old, extremes=ext, control=c17 if "control" in chosen else None, applied=a if "applied" in chosen else None,
                                         tether=net2 if "net" in chosen else None, peaks=peaks, implicit=implicit, ke=ke, **kw)
                    torch.cuda.synchronize()
                    return [state, prev, ke] + ([kw["log"]] if kw else []) + [x for x in (ext, peaks) if x is not None]
                peak_entry = lambda mooring: lambda cur, old, **kw: step(eng, "peak", cur, old, n, steps, step0=3, mooring=mooring, layers=2, **kw)  # noqa: E731
                spread_entry = lambda sp, layers: lambda cur, old, tether, **kw: step_spread(eng, cur, old, n, steps, step0=3, spread=sp, layers=layers,  # noqa: E731
                                                                                           tether=tether, net_layers=2, **kw)
                same = lambda x, y: all(_same_bits(p, q) for p, q in zip(x, y))  # noqa: E731
                want = run(peak_entry(None))
                assert same(run(spread_entry(None, 1)), want) and same(run(spread_entry(None, 9)), want), (n, steps, chosen)
                want = run(peak_entry(one))                       # (another kernel: _same_bits_or_nan)
                alike = lambda x, y: all(_same_bits_or_nan(p, q) for p, q in zip(x, y))  # noqa: E731
                got = run(spread_entry(one, 1))
                assert alike(got, want), (n, steps, chosen)
                assert alike(run(spread_entry(padded, 3)), want), (n, steps, chosen)
                # a NaN's bits may differ only in explicit 7-step runs, and only where both launches hold a NaN (alike, above)
                assert (steps == 7 and not implicit) or same(got, want), (n, steps, chosen)
                assert same(run(spread_entry(four, 4)), run(spread_entry(three, 3))), (n, steps, chosen)
        eng.close()


# ---- 3. the order of the additions -------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
@pytest.mark.parametrize("netted", [False, True], ids=["spread", "spread+net"])
def test_the_recorded_wrench_is_the_hosts_sum_in_ascending_layer_order(coeff, semantics, implicit, netted, pop, native_built):
    """One step over the bed, through the sea, every body watched with its wrench.  The logged wrench equals, bit for bit,
    fl(fl(fl(w + W_0) + W_1) + W_2) in fp32 on the host: w the logged wrench of the same step without lines, W_l the probe's
    output for layer l, a layer that does not pull skipped (no +0 is added) - and with a two-layer tether net BEHIND the spread
    the tether probe's outputs added behind those, in the net's layer order.  A body pulled in one layer only has the state of
    the link-tension entry's step with that layer alone as its record."""
    st, pv = pop["st"], pop["pv"]
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(sea)
        eng.set_seabed(BED)
        eng.set_watch(list(range(n)))
        spread = pop["spread"][:n]
        net = net_for(pop["net"], n, 2)
        tether = _tiled(net) if netted else None
        W = _probes(eng, st, spread, n, 4)
        T = _tensions_by_ext(eng, st, pv, spread, n, 4)
        pulls = np.stack([t > 0 for t in T])
        count = pulls.sum(axis=0)
        assert (count == 0).sum() >= 16 and (count == 1).sum() >= 16 and (count == 2).sum() >= 16 and (count == 3).sum() >= 2 and not pulls[3].any()
        assert all(np.array_equal(pulls[l], np.abs(W[l]).sum(axis=1) > 0) for l in range(4))

        def one(launch):
            log = torch.full((1, 19, n), NAN, dtype=torch.float32, device=DEV)
            cur, old = _buffers(st, pv, n)
            state, _ = launch(cur, old, implicit=implicit, log=log)
            torch.cuda.synchronize()
            return _from(state, n), log[0].cpu().numpy().T                                       # (n, 13), (n, 19)
        got_state, got_log = one(lambda cur, old, **kw: step_spread(eng, cur, old, n, 1, step0=7, spread=_tiled(spread), layers=4, tether=tether, net_layers=2, **kw))
        bare_state, bare_log = one(lambda cur, old, **kw: step(eng, "ext", cur, old, n, 1, step0=7, **kw))
        total = bare_log[:, 13:19].copy()
        for l in range(3):
            total = np.where(pulls[l][:, None], total + W[l], total)
        if netted:
            Wt, Tt = eng.tether_net_wrench(_tiled(st[:n]), _tiled(net), n, 2)
            for w, t in zip(Wt, Tt):
                total = np.where((_from(t, n)[:, 0] > 0)[:, None], total + _from(w, n), total)
        assert total.dtype == np.float32 and _same(np.ascontiguousarray(got_log[:, 13:19]), np.ascontiguousarray(total)), n
        assert _same(np.ascontiguousarray(got_log[:, 0:13]), got_state)
        if not netted:
            assert _same(got_state[count == 0], bare_state[count == 0])
        for l in range(3):
            rec = np.ascontiguousarray(spread[:, 9 * l:9 * l + 9])
            alone_state, alone_log = one(lambda cur, old, **kw: step(eng, "peak", cur, old, n, 1, step0=7, mooring=_tiled(rec), tether=tether, layers=2, **kw))
            only = pulls[l] & (count == 1)
            assert only.sum() >= (8, 8, 0)[l]
            assert _same(got_state[only], alone_state[only]) and _same(np.ascontiguousarray(got_log[only]), np.ascontiguousarray(alone_log[only])), (n, l)
        eng.close()


# ---- 4. the extremes record's tension -------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_tension_max_is_the_largest_tension_of_the_bodys_lines(coeff, implicit, pop, native_built):
    """After one step from an empty record tension_max equals, bit for bit, the maximum over the layers of the tension_max the
    extremes entry leaves with that layer's sub-record alone; after 7 steps, and after 7 x 1 and (2, 5) launches, the host's fold
    of those single-step values over steps and layers.  Everything else - state, prev_out, energy and log - does not depend on
    whether the extremes are tracked, and the position fields of the record are the fold of the recorded rows."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        watched = sorted({b for b in (0, 64, 72, 73, 80, 130, n - 1) if b < n})
        eng.set_watch(watched)
        spread = pop["spread"][:n]
        sp = _tiled(spread)
        T = _tensions_by_ext(eng, st, pv, spread, n, 4, implicit)
        top = np.argmax(np.stack(T), axis=0)
        count = np.stack([t > 0 for t in T]).sum(axis=0)
        assert all(((top == l) & (count >= 2)).sum() >= (8, 8, 2)[l] for l in range(3))     # no "layer 0 only", "last layer wins" or "sum" passes

        def run(chunks, tracked=True, fold=None):
            cur, old = _buffers(st, pv, n)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n) if tracked else None
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            ke = _ke()
            done = 0
            for k in chunks:
                if fold is not None:                              # the single-step values of the state this step starts from
                    s_now, pv_now = _from(cur, n), _from(old, n)[:, 7:13]
                    for t in _tensions_by_ext(eng, s_now, pv_now, spread, n, 3, implicit):
                        fold[:] = np.where(t > fold, t, fold)
                step_spread(eng, cur, old, n, k, step0=done, spread=sp, layers=4, extremes=ext, implicit=implicit, ke=ke, log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return [cur, old[:, 7:13], ke, log], ext
        first, ext1 = run([1])
        want1 = np.zeros(n, np.float32)
        for t in T:
            want1 = np.where(t > want1, t, want1)
        assert _same(np.ascontiguousarray(_from(ext1, n)[:, 7]), want1) and (want1 > 0).sum() >= n // 3, n
        fold = np.zeros(n, np.float32)
        singles, ext_singles = run([1] * 7, fold=fold)
        whole, ext_whole = run([7])
        chunks, ext_chunks = run([2, 5])
        untracked, _ = run([7], tracked=False)
        assert (fold >= want1).all()
        for ext in (ext_singles, ext_whole, ext_chunks):
            got = np.ascontiguousarray(_from(ext, n)[:, 7])
            ok = _same(got, fold) if implicit else bool(((got == fold) | (np.isnan(got) & np.isnan(fold))).all())
            assert ok, n
        assert _same_bits(ext_whole, ext_singles) and _same_bits(ext_whole, ext_chunks)
        for other in (singles, chunks, untracked):
            assert all(_same_bits(x, y) for x, y in zip(whole, other)), n
        rows = whole[3].cpu().numpy()                             # (7, 19, watched)
        e = _from(ext_whole, n)[watched]
        if implicit:
            for a in range(3):
                assert np.array_equal(e[:, 2 * a], rows[:, a, :].min(axis=0)) and np.array_equal(e[:, 2 * a + 1], rows[:, a, :].max(axis=0))
        eng.close()


# ---- 5. everything together against fp64 ---------------------------------------------------------------------------------------------
@COEFFS
def test_one_step_with_everything_against_fp64(coeff, pop, native_built):
    """Implicit drag + applied wrench + pose hold + sea with two waves + bed + the four-layer spread + a two-layer net.  Reference as
    in tests/test_tether_net_gpu.py, the lines' term the fp64 sum over the spread's layers; left out: bodies within 1e-4 of a
    branch of the hydrodynamic model, and the ties with a damper of layer 0 and of the net's layer 0."""
    st, pv, applied, ctl = pop["st"], pop["pv"], pop["applied"], pop["ctl"]
    pr = pop["params"][coeff]
    worst = {}
    sea = SeaState(SEA.current).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(sea)
        eng.set_seabed(BED)
        spread, net = pop["spread"][:n], net_for(pop["net"], n, 2)
        w = _from(eng.sea_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        keep[TIES[4:]] = False
        ties_c = np.asarray(bodies_of(pop["groups"], "ties_c"))
        keep[ties_c[ties_c < n]] = False
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step_spread(eng, cur, old, n, 1, step0=7, spread=_tiled(spread), layers=4, tether=_tiled(net), net_layers=2, control=_tiled(ctl[:n]),
                             applied=_tiled(applied[:n]), implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        on_m = [mr.taut_fp32(np.ascontiguousarray(rec), st[:n]) for rec in msr.layers_of(spread)]
        on_t = [tr.taut_fp32(rec, st[:n]) for rec in tnr.layers_of(net)]
        extra = br.wrench(BED, st[:n], pr[:n], touch) + msr.wrench(spread, st[:n], on_m) + tnr.wrench(net, st[:n], on_t)
        extra_scale = br.wrench_scales(BED, st[:n], pr[:n], touch) + msr.wrench_scales(spread, st[:n], on_m) + tnr.wrench_scales(net, st[:n], on_t)
        many = (msr.pulls(spread, st[:n]).sum(axis=0) >= 2) & keep
        assert many.sum() >= 16
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=extra[keep],
                                    bed_scale=extra_scale[keep])
        eng.close()
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[sea + applied + pose hold + bed + spread of 4 layers + net of 2, implicit, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g})")
    assert max(per_group.values()) <= B, worst


# ---- 6. step counts and the recorder -----------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    """7 steps = 7 x 1 = (2, 5) with step0 advanced: state, prev_out and every recorded row (state and wrench) of the watched
    bodies - bodies pulled in one, two and three layers among them - with a net, its link tensions and the extremes riding along."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        count = msr.pulls(pop["spread"][:n], st[:n]).sum(axis=0)
        watched = sorted({int(b) for c in (0, 1, 2, 3) for b in np.flatnonzero(count == c)[:4]} | {n - 1})
        assert {int(count[b]) for b in watched} == {0, 1, 2, 3}
        eng.set_watch(watched)
        sp, net2 = _tiled(pop["spread"][:n]), _tiled(net_for(pop["net"], n, 2))

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            ext, peaks = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
            done = 0
            for k in chunks:
                step_spread(eng, cur, old, n, k, step0=100 + done, spread=sp, layers=4, tether=net2, net_layers=2, peaks=peaks, extremes=ext, implicit=implicit,
                            log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, old[:, 7:13], log, ext, peaks
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
    bits of the temporal launch), with sea, bed, pose hold, applied wrench, the spread, a net and extremes active."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        sp, net2, a, c17 = _tiled(pop["spread"][:n]), _tiled(net_for(pop["net"], n, 2)), _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n])

        def run(ke=None, **kw):
            cur, old = _buffers(st, pv, n)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            state, prev = step_spread(eng, cur, old, n, 7, step0=5, spread=sp, layers=4, tether=net2, net_layers=2, extremes=ext, control=c17, applied=a,
                                      implicit=implicit, ke=ke, **kw)
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


# ---- 7. one row of the resident ladder ------------------------------------------------------------------------------------------------
def test_an_earlier_option_on_its_own_is_the_same_bits_through_the_spread_entry(pop, native_built):
    """tests/test_resident_ladder_gpu.py's row for the new entry: n = 65, 2 steps, f32, explicit, with the kinetic energy.  Each
    earlier option ON ITS OWN - log (through the link-tension entry), applied wrench (body frame), pose hold, sea, seabed, one mooring
    line per body, extremes, tether, two-layer net, link tensions (each through the entry that introduced it) - and through the
    spread entry: the same bits in everything the launch writes."""
    n, steps, step0 = 65, 2, 3
    st, pv = pop["st"], pop["pv"]
    own = dict(log="peak", applied="app", control="ctl", sea="sea", seabed="bed", mooring="moor", extremes="ext", tether="teth", net="net", peaks="peak")
    for option, entry in own.items():
        eng = _engine(n, pop["params"]["f32"], "f32")
        eng.set_watch([0, 5, 63, 64])
        eng.set_sea(SEA if option == "sea" else None)
        eng.set_seabed(BED if option == "seabed" else None)
        layers = 2 if option in ("net", "peaks") else 1

        def launch(through_spread):
            cur, old = _buffers(st, pv, n)
            ke = _ke()
            log = torch.full((steps, 19, 4), NAN, dtype=torch.float32, device=DEV) if option == "log" else None
            given = dict(applied=_tiled(pop["applied"][:n]) if option == "applied" else None,
                         control=_tiled(pop["ctl"][:n]) if option == "control" else None,
                         mooring=_tiled(np.ascontiguousarray(pop["spread"][:n, 0:9])) if option == "mooring" else None,
                         extremes=eng.extremes_reset(eng.alloc_tiled(8, n), n) if option == "extremes" else None,
                         tether=_tiled(net_for(pop["net"], n, layers)) if option in ("tether", "net", "peaks") else None,
                         peaks=eng.alloc_tiled(layers, n) if option == "peaks" else None)
            if through_spread:
                state, prev = step_spread(eng, cur, old, n, steps, step0=step0, spread=given["mooring"], layers=1, tether=given["tether"], net_layers=layers,
                                          peaks=given["peaks"], extremes=given["extremes"], applied=given["applied"], control=given["control"], frame="body",
                                          ke=ke, log=log)
            else:
                takes = ENTRIES[entry][1]
                state, prev = step(eng, entry, cur, old, n, steps, frame="body", ke=ke, log=log, step0=step0 if "step0" in takes else 0,
                                   layers=layers if "layers" in takes else None, **{k: v for k, v in given.items() if v is not None})
            torch.cuda.synchronize()
            return [state, prev, ke] + [x for x in (log, given["extremes"], given["peaks"]) if x is not None]
        want, got = launch(False), launch(True)
        assert len(got) == len(want) and all(_same_bits(x, y) for x, y in zip(got, want)), option
        eng.close()


# ---- 8. refusals and guards through the raw C ABI ------------------------------------------------------------------------------------
def test_refusals_launch_nothing(pop, native_built):
    """The link-tension entry's refusals first, then: layers outside 1 .. 4, a stride below 576 L, a misaligned record, the spread's
    last layer over state_out, over the extremes record and over tether_peaks."""
    n, L = 321, 3
    tiles, s_sp = (n + 63) // 64, S_SP(3)
    st, pv = pop["st"], pop["pv"]
    eng = _engine(n, pop["params"]["f32"], "f32")
    state, prev = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV)
    sp, net = _guarded(pop["spread"][:n, 0:27], s_sp), _guarded(net_for(pop["net"], n, 2), S_T2)
    # one allocation: the spread's copy at its head, and room behind it for an output that starts inside the last layer of its last tile
    inside = (tiles - 1) * s_sp + 576 * (L - 1) + 64
    arena = torch.full((inside + tiles * S_OUT,), NAN, device=DEV)
    arena[:tiles * s_sp] = sp
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    p2 = torch.full((tiles * S_P2,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    E_ARG = -1
    m, e, t = sp.data_ptr(), e8.data_ptr(), net.data_ptr()
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    call = lambda **kw: raw_spread(eng, n, state, prev, kw.pop("out", out), pvo, **{**dict(layers=L, s_mooring=s_sp, mooring=m), **kw})  # noqa: E731
    # the link-tension entry's own, in its order, before the spread's
    assert call(step0=-1) == (E_ARG, -7) and call(steps=0) == (E_ARG, -7)
    assert call(layers=0, extremes=e + 4) == (E_ARG, -7) and "mooring_layers" not in last()
    assert call(layers=0, tether=t, net_layers=5) == (E_ARG, -7) and "tether_layers" in last()
    assert call(layers=0, peaks=p2.data_ptr()) == (E_ARG, -7) and "tether_peaks without" in last()
    assert call(s_mooring=512) == (E_ARG, -7) and "mooring_layers" not in last()                    # below a single line's 576: the mooring's own refusal
    # the spread's
    for layers in (0, 5, -1):
        assert call(layers=layers) == (E_ARG, -7) and "mooring_layers" in last(), layers
    assert raw_spread(eng, n, state, prev, out, pvo, layers=5, mooring=None, s_mooring=0)[0] == 0    # without a spread the layers are not looked at
    assert call(s_mooring=576 * L - 64) == (E_ARG, -7) and "stride" in last()
    assert call(layers=4) == (E_ARG, -7) and "stride" in last()                                     # the stride of three layers is below 576 * 4
    assert call(mooring=m + 4) == (E_ARG, -7)                                                      # misaligned
    assert call(layers=2)[0] == 0                                                                  # (and is any stride for two)
    head = arena.data_ptr()
    assert call(mooring=head, out=head + 4 * inside) == (E_ARG, -7) and "must not overlap" in last()
    assert call(mooring=head, extremes=head + 4 * inside) == (E_ARG, -7) and "must not overlap" in last()
    assert call(mooring=head, tether=t, peaks=head + 4 * inside) == (E_ARG, -7) and "must not overlap" in last()
    torch.cuda.synchronize()
    out[:] = NAN                                                   # (the accepted launches above wrote state_out and prev_out)
    pvo[:] = NAN
    for layers in (0, 5, -1):
        assert call(layers=layers) == (E_ARG, -7)
    assert call(s_mooring=576 * L - 64) == (E_ARG, -7) and call(mooring=m + 4) == (E_ARG, -7)
    assert call(mooring=head, out=head + 4 * inside) == (E_ARG, -7)
    assert call(mooring=head, extremes=head + 4 * inside) == (E_ARG, -7)
    assert call(mooring=head, tether=t, peaks=head + 4 * inside) == (E_ARG, -7)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(e8).all() and torch.isnan(p2).all()
    assert torch.isnan(arena[tiles * s_sp:]).all() and _untouched(arena[:tiles * s_sp], sp.cpu().numpy())
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64 and different for every buffer - the spread's 576 L + 52 - NaN in the stride
    padding and past body n of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or
    overwritten, and the inputs, the spread with its sentinels included, are untouched."""
    st, pv = pop["st"], pop["pv"]
    n, tiles, L = 200, 4, 3
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    rec, net = pop["spread"][:n, 0:27], net_for(pop["net"], n, 2)
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m27, t14 = _guarded(rec, S_SP(L)), _guarded(net, S_T2)
    empty = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32), (n, 1))
    e8, p2 = _guarded(empty, S_E), _guarded(np.zeros((n, 2), np.float32), S_P2)
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m27, t14)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    rc, written = raw_spread(eng, n, state, prev, out, pvo, layers=L, s_mooring=S_SP(L), mooring=m27.data_ptr(), steps=3, step0=11, implicit=implicit, log=log,
                             applied=a.data_ptr(), control=c17.data_ptr(), extremes=e8.data_ptr(), tether=t14.data_ptr(), peaks=p2.data_ptr())
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    ext, erest = _unguard(e8, n, 8, S_E)
    peaks, krest = _unguard(p2, n, 2, S_P2)
    assert all(np.isnan(r).all() for r in (rest, prest, erest, krest)), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m27, t14), before))
    assert np.isfinite(got).all() or not implicit, "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want_ext, want_peaks = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
    want, want_prev = step_spread(eng, cur, old, n, 3, step0=11, spread=_tiled(rec), layers=L, tether=_tiled(net), net_layers=2, peaks=want_peaks,
                                  extremes=want_ext, control=_tiled(pop["ctl"][:n]), applied=_tiled(pop["applied"][:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert _same(got, _from(want, n)) and _same(pv_out, _from(want_prev, n)) and _same(ext, _from(want_ext, n)) and _same(peaks, _from(want_peaks, n))
    assert (ext[:, 7] > 0).sum() >= n // 3
    eng.close()


@COEFFS
@DRAG
def test_a_malformed_layer_is_computed_as_given_and_is_its_own_bodys_problem(coeff, implicit, pop, native_built):
    """tests/value_contract.py's table of malformed mooring lines (k NaN, negative, +Inf; c negative; L0 NaN, +-Inf, negative; a NaN
    fairlead), built on layer 0's pulling lines and placed in LAYER 2 behind the designed layers 0 and 1: the probe of that layer
    gives the bits of the probe on the malformed record alone (computed as given, no validation on the device), and a step
    leaves every body that is not a case lane with the bits of the step whose layer 2 holds the clean lines."""
    import value_contract as vc
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_watch(list(range(n)))
        rec0 = pop["spread"][:, 0:9]
        pulling = np.flatnonzero(population_report(rec0, st)[0] & OFF_TIES)
        table = vc.malformed_lines(rec0, st, pulling, n)
        assert table.lanes.sum() >= 10
        front = pop["spread"][:n, 0:18]
        bad, clean = np.concatenate([front, table.bad], axis=1), np.concatenate([front, table.clean], axis=1)
        W = _probes(eng, st, bad, n, 3)
        assert _same(W[2], _from(eng.mooring_wrench(_tiled(st[:n]), _tiled(table.bad), n), n)), n
        assert all(_same(x, y) for x, y in zip(W[:2], _probes(eng, st, clean, n, 3)[:2]))          # the layers in front do not see it

        def run(spread):
            cur, old = _buffers(st, pv, n)
            log = torch.full((3, 19, n), NAN, dtype=torch.float32, device=DEV)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            state, prev = step_spread(eng, cur, old, n, 3, spread=_tiled(spread), layers=3, extremes=ext, implicit=implicit, log=log)
            torch.cuda.synchronize()
            return _from(state, n), _from(prev, n), _from(ext, n), np.ascontiguousarray(log.cpu().numpy().transpose(2, 0, 1).reshape(n, -1))
        others = ~table.lanes
        for got, want in zip(run(bad), run(clean)):
            assert np.array_equal(np.ascontiguousarray(got[others]).view(np.uint32), np.ascontiguousarray(want[others]).view(np.uint32)), n
        eng.close()


# ---- 9. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 322, the last tile with two live lanes) on three lines each, drawn round every body, 0.1 m short."""
    sc = scenes.scene_c2(n=322)
    m = sc.params[:, 10].astype(np.float64)
    rng = np.random.default_rng(11)
    centre = sc.state[:, 0:2].astype(np.float64)
    phi = rng.uniform(0.0, 2.0 * np.pi, 322)[:, None] + 2.0 * np.pi * np.arange(3)[None, :] / 3.0
    anchors = np.stack([centre[:, None, 0] + 6.0 * np.cos(phi), centre[:, None, 1] + 6.0 * np.sin(phi),
                        np.broadcast_to(sc.state[:, None, 2].astype(np.float64) - 8.0, (322, 3))], axis=2)
    k, c = MooringSpread.for_body(m, sc.dt, 3)
    return sc, dict(anchors=anchors, length=9.9, stiffness=np.repeat(k[:, None], 3, axis=1), damping=np.repeat(c[:, None], 3, axis=1))


def test_sim_runners_and_a_graph_replay_agree_with_a_spread_set_and_clear_gives_the_sim_back(native_built):
    sc, lines = _scene()
    finals, tension = {}, {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.set_sea(SeaState((0.4, -0.1, 0.0)))
        buf = sim.set_mooring_spread(**lines)
        sim.track_extremes()
        assert buf is sim.mooring_spread and sim.mooring_layers == 3 and tuple(buf.shape) == (6, 27, 64)
        go(sim)
        assert name != "graph" or sim._graph is not None
        finals[name], tension[name] = sim.state(), sim.extremes.tension_max()
        sim.close()
    for name in ("resident", "chunks", "graph"):
        assert _same(finals["eager"], finals[name]) and _same(tension["eager"], tension[name]), name
    assert (tension["eager"] > 0).mean() > 0.9
    never, cleared = ClosedLoopSim(sc, implicit_drag=True), ClosedLoopSim(sc, implicit_drag=True)
    cleared.set_mooring_spread(**lines)
    cleared.clear_mooring_spread()
    assert cleared.mooring_spread is None and cleared.mooring_layers == 0
    for s in (never, cleared):
        s.run_resident(32)
        s.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state()) and not np.array_equal(never.state(), finals["eager"])
    cleared.set_mooring_spread(**lines)
    with pytest.raises(ValueError, match=r"clear_mooring_spread\(\) first"):
        cleared.set_mooring(anchor=(0.0, 0.0, -5.0), length=1.0, stiffness=1.0)
    waves = ClosedLoopSim(sc, implicit_drag=True)
    waves.set_mooring_spread(**lines)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    for s in (never, cleared, waves):
        s.close()


# ---- 10. the physical cases of tests/test_mooring_spread.py on the device ------------------------------------------------------------
RADIUS, ANCHOR_DEPTH = 15.0, 20.0
SETTLE_STEPS, SETTLE_LAST, SETTLE_XY, SETTLE_Z, SETTLE_SPEED = 1800, 60, 1e-9, 2 * 1.1e-6, 2 * 6.5e-6   # tests/test_mooring_spread.py's figures
STATION_STEPS, STATION_EXCURSION, WATCH_CIRCLE = 3600, 0.522, 2.56


def _copies():
    """64 copies of config 1's buoy at rest at its draught, 50 m apart."""
    st, pv, pr, sc, dt, z_eq, mass = buoy()
    i = np.arange(64)
    st, pv, pr = np.tile(st, (64, 1)), np.tile(pv, (64, 1)), np.tile(pr, (64, 1))
    st[:, 0], st[:, 1] = 50.0 * (i % 8), 50.0 * (i // 8)
    return st, pv, pr, sc, dt, z_eq, mass


def test_four_symmetric_lines_settle_64_buoys_at_the_analytic_depth(native_built):
    st, pv, pr, sc, dt, z_eq, mass = _copies()
    k, c = MooringSpread.for_body(mass, dt, 4)
    L0 = float(np.float32(np.hypot(RADIUS, ANCHOR_DEPTH + z_eq) - 0.5))
    cross = np.array([[RADIUS, 0.0], [0.0, RADIUS], [-RADIUS, 0.0], [0.0, -RADIUS]])
    anchors = np.concatenate([st[:, None, 0:2].astype(np.float64) + cross[None], np.full((64, 4, 1), -ANCHOR_DEPTH)], axis=2)
    sim = ClosedLoopSim(scenes.Scene("buoys on four lines", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g), implicit_drag=True)
    sim.set_mooring_spread(anchors, length=L0, stiffness=k, damping=c)
    # the figures are those of the LAST SECOND (the heave decays through zero crossings: one instant says nothing), and the extremes
    # record, emptied a second before the end, is what keeps them on the device
    sim.run_resident(SETTLE_STEPS - SETTLE_LAST, chunk=60)
    box = sim.track_extremes(from_state=False)
    sim.run_resident(SETTLE_LAST, chunk=60)
    e = box.bodies().astype(np.float64)
    sim.close()
    f = lambda z: 4.0 * k * (np.hypot(RADIUS, ANCHOR_DEPTH + z) - L0) * (ANCHOR_DEPTH + z) / np.hypot(RADIUS, ANCHOR_DEPTH + z) - (sc.rho * sc.g * (0.5 - z) - mass * sc.g)  # noqa: E731
    lo, hi = -0.5, 0.5
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0.0 else (lo, mid)
    z_want = 0.5 * (lo + hi)
    centre = st[:, 0:2].astype(np.float64)
    off_xy = max(np.abs(e[:, 0:2] - centre[:, 0:1]).max(), np.abs(e[:, 2:4] - centre[:, 1:2]).max())
    off_z, speed = np.abs(e[:, 4:6] - z_want).max(), float(np.sqrt(e[:, 6].max()))
    print(f"[four lines on the device, 64 copies, last {SETTLE_LAST} steps] |x|, |y| <= {off_xy:.1e} m  |z - root| <= {off_z:.2e} m (threshold {SETTLE_Z:g})  "
          f"|v| <= {speed:.2e} m/s (threshold {SETTLE_SPEED:g})")
    assert off_xy <= SETTLE_XY and off_z <= SETTLE_Z and speed <= SETTLE_SPEED


def test_three_lines_keep_64_buoys_on_station_where_one_line_gives_a_watch_circle(native_built):
    st, pv, pr, sc, dt, z_eq, mass = _copies()
    theta = 2.0 * np.pi * (np.arange(64) % 8) / 8.0                # the current from eight headings: the spread and the buoy turned against it
    st[:, 5], st[:, 6] = np.sin(-0.5 * theta), np.cos(-0.5 * theta)
    centre = st[:, 0:2].astype(np.float64)
    scene = scenes.Scene("buoys on three lines", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g)
    k3, c3 = MooringSpread.for_body(mass, dt, 3)
    phi = -theta[:, None] + 2.0 * np.pi * np.arange(3)[None, :] / 3.0
    anchors = np.stack([centre[:, None, 0] + RADIUS * np.cos(phi), centre[:, None, 1] + RADIUS * np.sin(phi), np.full((64, 3), -ANCHOR_DEPTH)], axis=2)
    spread, single = ClosedLoopSim(scene, implicit_drag=True), ClosedLoopSim(scene, implicit_drag=True)
    spread.set_mooring_spread(anchors, length=np.hypot(RADIUS, ANCHOR_DEPTH + z_eq) - 0.1, stiffness=k3, damping=c3)
    k1, c1 = Mooring.for_body(mass, dt)
    single.set_mooring(np.concatenate([centre, np.full((64, 1), z_eq - DEPTH)], axis=1), length=DEPTH + 0.5, stiffness=k1, damping=c1)
    for s in (spread, single):
        s.set_sea(SeaState((0.5, 0.0, 0.0)))
    box = spread.track_extremes()
    spread.run_resident(STATION_STEPS, chunk=64)
    single.run_resident(STATION_STEPS, chunk=64)
    # the largest excursion over the run is inside the box the extremes record kept: its far corner bounds it from above
    corner = box.excursion(centre)
    final = np.linalg.norm(spread.state()[:, 0:2].astype(np.float64) - centre, axis=1)
    circle = single.state()[:, 0].astype(np.float64) - centre[:, 0]
    print(f"[three lines on the device, 64 copies] final excursion {final.min():.3f} .. {final.max():.3f} m, box corner <= {corner.max():.3f} m; one line: "
          f"{circle.min():.3f} .. {circle.max():.3f} m downstream")
    assert corner.max() <= STATION_EXCURSION and final.max() <= STATION_EXCURSION
    assert (circle >= WATCH_CIRCLE).all() and circle.min() >= 5.0 * corner.max()
    assert (box.tension_max() > 0).all()
    for s in (spread, single):
        s.close()


def test_spread_moored_buoy_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "spread_moored_buoy.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    m = re.search(r"largest excursion on three lines ([\d.]+) m, on one line ([\d.]+) m", res.stdout)
    assert m and float(m.group(1)) < float(m.group(2)), res.stdout
    assert re.search(r"tension_max \(N\):((?: +[\d.]+)+)", res.stdout)
