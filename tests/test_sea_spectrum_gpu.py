"""Irregular seas on the device (hydro_set_sea_spectrum, hydro_sea_spectrum_sample, hydro_step_fused_tiled_multi_irr).  THE
YARDSTICK: for up to 8 components the spectrum's water is the regular sea's, bit for bit - the sample against hydro_sea_sample,
the step against hydro_step_fused_tiled_multi_spread under hydro_set_sea, in everything a launch writes.  Above 8 components
the sample follows the fp64 restatement of tests/sea_reference.py within SPECTRUM_VIEW_BOUND, which
tests/sea_spectrum_reference.py derives on the host (E = 1.90 units emulated, bound 4) - and the same reference with one
component removed misses by more than ten bounds; an explicit step is, bit for bit, the wrench kernel on the relative state built
from the sample followed by the integrator kernel on the true one - at 64 components and at 9, 10, 11 and 63, which leave the loop's
groups of four a remainder; one implicit step at 11 and 64 components follows the fp64 step within integrator_oracle.STEP_ULP_BOUND;
the phase advances inside a launch; trailing components of
amplitude 0 change no bit; refusals, guards, ClosedLoopSim's runners, the example.

Sizes: n = 65 (two tiles, ONE live lane in the second: a scheme in which lanes compute phases for each other would fail there),
200 and 321.  The designed spectrum (sea_spectrum_reference.designed_spectrum): equal amplitudes, a direction and a frequency of
its own per component."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sea_reference as sr
import sea_spectrum_reference as ssr
from conftest import REPO
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import jonswap, SeaSpectrum, SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from mooring_spread_population import spread_population
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, RHO, S_A, S_C,
                              S_IN, S_OUT, S_PV, S_PVO, _same, _same_bits, _tiled, _unguard, _untouched, _watched)
from tether_net_population import net_for, net_population

pytestmark = pytest.mark.gpu
SIZES = (65, 200, 321)
WATCH = (0, 63, 64)
BOUND = ssr.SPECTRUM_VIEW_BOUND
FULL = ssr.designed_spectrum()                                    # 64 components, U = (0.5, -0.2, 0.05)
S_W = 4 * 64 + 52                                                 # the sample's tile stride in the guard tests
REMAINDERS = (9, 10, 11, 63)                                      # component counts that leave 1, 2 and 3 trips behind the groups of four
S_E, S_T2, S_P2, S_SP3 = 8 * 64 + 36, 448 * 2 + 44, 64 * 2 + 20, 576 * 3 + 52      # extremes, a two-layer net, its link tensions, a spread of three


def _as_sea(spec):
    """The regular sea of the same current and components (at most 8)."""
    sea = SeaState(spec.current)
    for w in spec.waves:
        sea.add_wave(*w)
    return sea


@pytest.fixture(scope="module")
def vpop(hold_pop):
    """Section 15's designed population (coordinates out to 1e4 m), its first 321 bodies, moved onto the surface the designed
    spectrum displaces."""
    st, pv, params, applied, ctl, _ = hold_pop
    n = max(SIZES)
    st = ssr.spectrum_population(st[:n], FULL)
    eta, _ = sr.water(FULL, st[:, 0], st[:, 1], st[:, 2], 0, DT)
    ext = scenes.vertical_extent(st[:, 3:7], params["f32"][:n, 0:3])
    z_rel = st[:, 2] - eta
    assert (np.abs(z_rel) < ext).mean() >= 1 / 3 and (z_rel < -ext).mean() >= 1 / 3
    return st, pv[:n], {k: v[:n] for k, v in params.items()}, applied[:n], ctl[:n]


@pytest.fixture(scope="module")
def pop(bed_pop):
    """tests/test_mooring_spread_gpu.py's population: 321 bodies over the bed with the designed spread and the tether net."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, _ = net_population()
    st, pv = st[:321], pv[:321]
    spread = spread_population(st, params["f32"], line_population(st, params["f32"]))
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, spread=spread, net=net)


def _launch(eng, which, cur, old, n, steps, *, step0=0, spread=None, layers=1, tether=None, net_layers=1, peaks=None, extremes=None, applied=None,
            frame="world", control=None, implicit=False, ke=None, **kw):
    """One launch of the _irr or the _spread entry through the engine: (state, prev_out)."""
    getattr(eng, "step_fused_tiled_multi_" + which)(cur, old, n, DT, steps, step0, spread, layers, tether, net_layers, peaks, extremes, control, applied, frame,
                                                    implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def _sample(eng, st, n, step, spectrum=True):
    fn = eng.sea_spectrum_sample if spectrum else eng.sea_sample
    return fn(_tiled(st[:n]), n, step, DT)


# ---- 1. the sample is the regular sea's --------------------------------------------------------------------------------------------
def test_sample_is_the_regular_seas_up_to_eight_components(vpop, native_built):
    """1 and 8 components, and the first 8 of 9 (the ninth with amplitude 0: nine trips of the loop, the eight-component sum)."""
    st = vpop[0]
    nine = ssr.truncated(FULL, 8).add_wave(0.0, *FULL.waves[8][1:])
    for spec, sea in ((ssr.truncated(FULL, 1), None), (ssr.truncated(FULL, 8), None), (nine, _as_sea(ssr.truncated(FULL, 8)))):
        sea = sea or _as_sea(spec)
        for n in SIZES:
            eng = _engine(n, vpop[2]["f32"], "f32")
            eng.set_sea(sea)
            want = [_sample(eng, st, n, step, spectrum=False) for step in ssr.VIEW_STEPS]
            eng.set_sea(None)
            eng.set_sea_spectrum(spec)
            for step, w in zip(ssr.VIEW_STEPS, want):
                got = _sample(eng, st, n, step)
                torch.cuda.synchronize()
                assert _same_bits(got, w), (len(spec.waves), n, step)
                assert float(_from(got, n)[:, 0].std()) > 0.0 or n == 1
            eng.close()


# ---- 2. the sample against fp64 -----------------------------------------------------------------------------------------------------
def test_sample_against_the_fp64_restatement(vpop, native_built):
    st = vpop[0]
    worst = {"eta": 0.0, "u": 0.0, "z_rel": 0.0}
    dropped = np.inf
    for count in (9, 16, 17, 63, 64):
        spec = ssr.truncated(FULL, count)
        for n in SIZES:
            eng = _engine(n, vpop[2]["f32"], "f32")
            eng.set_sea_spectrum(spec)
            for step in ssr.VIEW_STEPS:
                got = _from(_sample(eng, st, n, step), n)
                for k, v in ssr.view_errors(spec, st[:n], step, DT, got[:, 0], got[:, 1:4]).items():
                    worst[k] = max(worst[k], v)
                if count == 64:                                  # a reference that lacks component 63 is told apart at every size and step
                    miss = ssr.view_errors(ssr.without(spec, 63), st[:n], step, DT, got[:, 0], got[:, 1:4])
                    dropped = min(dropped, miss["eta"], miss["u"])
            eng.close()
    print("[spectrum view] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {BOUND:g}); without component 63 the reference misses by {dropped:.3g}")
    assert max(worst.values()) <= BOUND, worst
    assert dropped > 10 * BOUND


# ---- 3. the step is the spread entry's ----------------------------------------------------------------------------------------------
def test_without_a_spectrum_every_option_on_its_own_is_the_spread_entrys_bits(pop, native_built):
    """The ladder row of the entry: n = 65, 2 steps, f32, explicit, with the kinetic energy; each option alone - and none."""
    n, steps, step0 = 65, 2, 3
    st, pv = pop["st"], pop["pv"]
    sea8 = _as_sea(ssr.truncated(FULL, 8))
    for option in (None, "log", "applied", "control", "sea", "seabed", "spread", "extremes", "net", "peaks"):
        eng = _engine(n, pop["params"]["f32"], "f32")
        eng.set_watch([0, 5, 63, 64])
        eng.set_sea(sea8 if option == "sea" else None)
        eng.set_seabed(BED if option == "seabed" else None)
        layers = 2 if option in ("net", "peaks") else 1

        def launch(which):
            cur, old = _buffers(st, pv, n)
            ke = _ke()
            log = torch.full((steps, 19, 4), NAN, dtype=torch.float32, device=DEV) if option == "log" else None
            extremes = eng.extremes_reset(eng.alloc_tiled(8, n), n) if option == "extremes" else None
            peaks = eng.alloc_tiled(layers, n) if option == "peaks" else None
            state, prev = _launch(eng, which, cur, old, n, steps, step0=step0, spread=_tiled(pop["spread"][:n, 0:27]) if option == "spread" else None, layers=3,
                                  tether=_tiled(net_for(pop["net"], n, layers)) if option in ("net", "peaks") else None, net_layers=layers, peaks=peaks,
                                  extremes=extremes, applied=_tiled(pop["applied"][:n]) if option == "applied" else None,
                                  control=_tiled(pop["ctl"][:n]) if option == "control" else None, frame="body", ke=ke, log=log)
            torch.cuda.synchronize()
            return [state, prev, ke] + [x for x in (log, extremes, peaks) if x is not None]
        want, got = launch("spread"), launch("irr")
        assert len(got) == len(want) and all(_same_bits(x, y) for x, y in zip(got, want)), option
        eng.close()


def _everything(eng, which, pop, n, steps, step0, implicit, ke=None, bare=False, **kw):
    """A launch with the spread of three, the two-layer net with its link tensions, extremes, pose hold, applied wrench and a log -
    or, bare, with nothing.  Returns everything it wrote."""
    cur, old = _buffers(pop["st"], pop["pv"], n)
    if bare:
        state, prev = _launch(eng, which, cur, old, n, steps, step0=step0, implicit=implicit, ke=ke, **kw)
        torch.cuda.synchronize()
        return [state, prev] + ([ke] if ke is not None else [])
    watched = _watched(n, WATCH)
    eng.set_watch(watched)
    log = torch.full((steps, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
    extremes, peaks = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
    state, prev = _launch(eng, which, cur, old, n, steps, step0=step0, spread=_tiled(pop["spread"][:n, 0:27]), layers=3, tether=_tiled(net_for(pop["net"], n, 2)),
                          net_layers=2, peaks=peaks, extremes=extremes, applied=_tiled(pop["applied"][:n]), control=_tiled(pop["ctl"][:n]), frame="body",
                          implicit=implicit, ke=ke, log=log, **kw)
    torch.cuda.synchronize()
    return [state, prev, log, extremes, peaks] + ([ke] if ke is not None else [])


def _same_or_nan(a, b):
    """Bit for bit, but that a NaN equals a NaN whatever its payload (seven explicit steps carry a light, strongly damped body of the
    population out of the fp32 range)."""
    i = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(((a.contiguous().view(i) == b.contiguous().view(i)) | (torch.isnan(a) & torch.isnan(b))).all())


@COEFFS
@DRAG
def test_a_spectrum_of_up_to_eight_components_is_the_spread_entry_under_the_same_sea(coeff, implicit, pop, native_built):
    """state_out, prev_out, the log, the extremes, the link tensions and the energy pair; 1 and 8 components; everything on, and nothing."""
    for count in (1, 8):
        spec = ssr.truncated(FULL, count)
        for n in SIZES:
            eng = _engine(n, pop["params"][coeff], coeff)
            eng.set_seabed(BED)
            for bare in (False, True):
                eng.set_sea_spectrum(None)
                eng.set_sea(_as_sea(spec))
                want = _everything(eng, "spread", pop, n, 7, 5, implicit, ke=_ke(), bare=bare)
                still = _everything(eng, "spread", pop, n, 7, 5, implicit, bare=bare) if bare else None
                eng.set_sea(None)
                if bare:                                         # the sea acts: without it the bodies end elsewhere
                    calm = _everything(eng, "spread", pop, n, 7, 5, implicit, bare=True)
                    assert not _same_or_nan(calm[0], still[0]), (count, n)
                eng.set_sea_spectrum(spec)
                got = _everything(eng, "irr", pop, n, 7, 5, implicit, ke=_ke(), bare=bare)
                assert len(got) == len(want) and all(_same_or_nan(x, y) for x, y in zip(got, want)), (count, n, bare)
            eng.close()


@COEFFS_SEMANTICS
def test_energy_and_non_temporal_instantiations(coeff, semantics, pop, native_built):
    """KE = true and NT = true (set_tuning(0, 0, 1)) in both semantics, once each, at 64 components with everything on: the bits of the
    launch without sampling and of the temporal launch; with implicit drag the energy pair against fp64 to 1e-12."""
    n = 321
    eng = _engine(n, pop["params"][coeff], coeff, semantics)
    eng.set_seabed(BED)
    eng.set_sea_spectrum(FULL)
    eng.set_tuning(0, 0, 0)
    want = _everything(eng, "irr", pop, n, 7, 5, True)
    ke = _ke()
    got = _everything(eng, "irr", pop, n, 7, 5, True, ke=ke)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    state = _from(got[0], n)
    assert np.isfinite(state).all()
    lin, rot = scenes.kinetic_energy_fp64(state, pop["params"][coeff][:n], rotational=True)
    pair = ke.cpu().tolist()
    assert lin > 0 and rot > 0 and pair[0] == pytest.approx(lin, rel=1e-12) and pair[1] == pytest.approx(rot, rel=1e-12)
    eng.set_tuning(0, 0, 1)
    ke_nt = _ke()
    streamed = _everything(eng, "irr", pop, n, 7, 5, True, ke=ke_nt)
    assert all(_same_bits(x, y) for x, y in zip(streamed, got))
    assert all(_same_bits(x, y) for x, y in zip(_everything(eng, "irr", pop, n, 7, 5, True), want))
    eng.close()


# ---- 4. the explicit step, composed ---------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_explicit_step_is_wrench_of_the_relative_state_then_integrator_of_the_true_one(coeff, semantics, vpop, native_built):
    """All 64 components at every size from steps 0 and 7 and, at n = 65 from step 7, the first 9, 10, 11 and 63: the component loops
    are unrolled in groups of four, and 64 is a multiple of four - one, two and three remainder trips behind two groups, and three
    behind fifteen, in the STEP kernel's instantiation of spectrum_water (the sample kernel's is another one, under another
    register budget).  The yardstick is the same composition, bit for bit; the sample itself is held to fp64 at these counts by
    test_sample_against_the_fp64_restatement."""
    st, pv, params, _, _ = vpop
    cases = [(FULL, n, (0, 7)) for n in SIZES] + [(ssr.truncated(FULL, count), 65, (7,)) for count in REMAINDERS]
    assert [len(spec.waves) for spec, _, _ in cases[len(SIZES):]] == list(REMAINDERS)
    for spec, n, starts in cases:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea_spectrum(spec)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)
        what = (len(spec.waves), n)
        for step0 in starts:
            w = _from(_sample(eng, st, n, step0), n)
            s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
            assert (s_rel[:, 2] != st[:n, 2]).mean() > 0.9
            wrench = eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel))
            cur, old = _buffers(st, pv, n)
            want = eng.integrate_tiled(cur, wrench, n, DT)
            log = torch.full((1, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            got, got_prev = _launch(eng, "irr", cur, old, n, 1, step0=step0, log=log)
            torch.cuda.synchronize()
            assert _same_bits(got, want), what + (step0,)
            assert np.array_equal(got_prev.cpu().numpy().view(np.uint32), scenes.to_tiled(st[:n, 7:13]).view(np.uint32))    # the TRUE velocity
            host = log.cpu().numpy()[0]
            assert np.array_equal(host[:13].T.view(np.uint32), _from(want, n)[watched].view(np.uint32)), what + (step0,)
            assert np.array_equal(host[13:].T.view(np.uint32), _from(wrench, n)[watched].view(np.uint32)), what + (step0,)
        eng.close()


# ---- 4b. one implicit step against fp64 -----------------------------------------------------------------------------------------------
@COEFFS
@pytest.mark.parametrize("count", [11, 64])
def test_implicit_step_above_eight_components_against_fp64(count, coeff, vpop, native_built):
    """One implicit step of the _irr entry with no other option on, at 11 (two groups of four and three remainder trips) and 64
    components, n = 65, 200 and 321 - above 8 components the implicit-drag instantiations are otherwise compared with themselves
    only.  The construction of tests/test_step_variants_gpu.py's test_body_frame_applied_wrench_in_waves_against_fp64: the relative
    state formed on the host from hydro_sea_spectrum_sample, the device's hydrodynamic wrench of it (hydro_step_wrench_tiled), the
    drag coefficients of integrator_oracle.drag_jacobian on the relative state, and integrator_oracle.integrate of the TRUE state
    through resident_harness.fp64_step_errors; left out, as there: bodies within 1e-4 of a branch of the hydrodynamic model.
    Bound: integrator_oracle.STEP_ULP_BOUND.  On an MI355X: see DESIGN.md section 29."""
    st, pv, params, _, _ = vpop
    pr = params[coeff]
    spec = ssr.truncated(FULL, count)
    step0 = 7
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea_spectrum(spec)
        w = _from(_sample(eng, st, n, step0), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8 and (s_rel[:, 2] != st[:n, 2]).mean() > 0.9, (n, keep.mean())
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = _launch(eng, "irr", cur, old, n, 1, step0=step0, implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        k = _k(ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2], s_rel, pr, coeff, n)
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], (k[0][keep], k[1][keep]))
        eng.close()
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[one implicit step, {count} components, no other option, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g}); worst {max(per_group.values()):.2f}")
    assert max(per_group.values()) <= B, worst


# ---- 5. time advances inside the launch --------------------------------------------------------------------------------------------
@COEFFS
@DRAG
@pytest.mark.parametrize("start", [0, 10 ** 6])
def test_one_launch_equals_single_steps_and_chunks_and_differs_from_a_frozen_phase(coeff, implicit, start, vpop, native_built):
    st, pv, params, _, _ = vpop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea_spectrum(FULL)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)

        def run(chunks, frozen=False):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 13, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                _launch(eng, "irr", cur, old, n, k, step0=start if frozen else start + done, implicit=implicit, log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, old[:, 7:13], log
        one, singles, chunks, frozen = run([7]), run([1] * 7), run([2, 5]), run([1] * 7, frozen=True)
        for other in (singles, chunks):
            assert all(_same_or_nan(x, y) for x, y in zip(one, other)), (n, start)
        finite = torch.isfinite(one[0]).all(dim=1, keepdim=True) & torch.isfinite(frozen[0]).all(dim=1, keepdim=True)
        # a view evaluated once per launch would give `frozen`: the same first step, then apart
        assert _same_bits(one[2][0], frozen[2][0]) and not _same_or_nan(one[2][1], frozen[2][1]), (n, start)
        assert bool(((one[0] != frozen[0]) & finite).any()), (n, start)
        eng.close()


# ---- 6. components of amplitude 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("current", [(0.0, 0.0, 0.0), (0.5, -0.2, 0.05)], ids=["U=+0", "U"])
def test_trailing_components_of_amplitude_zero_change_no_bit(current, vpop, native_built):
    """17 components, then the same with 30 more of amplitude 0 (wave vectors and frequencies of their own), then with 47 of them."""
    st, pv, params, _, _ = vpop
    base = SeaSpectrum(current)
    for w in FULL.waves[:17]:
        base.add_wave(*w)
    n = 200
    eng = _engine(n, params["f32"], "f32")
    want = None
    for extra in (0, 30, 47):
        spec = SeaSpectrum(current)
        for w in base.waves:
            spec.add_wave(*w)
        for w in FULL.waves[17:17 + extra]:
            spec.add_wave(0.0, *w[1:])
        eng.set_sea_spectrum(spec)
        cur, old = _buffers(st, pv, n)
        ke = _ke()
        state, prev = _launch(eng, "irr", cur, old, n, 3, step0=11, implicit=True, ke=ke)
        got = [_sample(eng, st, n, 11), state, prev, ke]
        torch.cuda.synchronize()
        want = want or got
        assert all(_same_bits(x, y) for x, y in zip(got, want)), extra
    # a spectrum with no current and nothing but components of amplitude 0 is still water: the spread entry's bits without a sea
    if current == (0.0, 0.0, 0.0):
        flat = SeaSpectrum()
        for w in FULL.waves:
            flat.add_wave(0.0, *w[1:])
        eng.set_sea_spectrum(flat)
        cur, old = _buffers(st, pv, n)
        got = _launch(eng, "irr", cur, old, n, 3, step0=11, implicit=True)
        cur, old = _buffers(st, pv, n)
        still = _launch(eng, "spread", cur, old, n, 3, step0=11, implicit=True)
        torch.cuda.synchronize()
        assert _same_bits(got[0], still[0]) and _same_bits(got[1], still[1])
    eng.close()


# ---- 7. refusals through the raw C ABI -------------------------------------------------------------------------------------------------
def _c_spectrum(spec, count=None):
    rows = (nat.SeaWave * max(len(spec.waves), 1))(*[nat.SeaWave(*w) for w in spec.waves])
    c = nat.SeaSpectrum()
    c.current[:] = spec.current
    c.waves = len(spec.waves) if count is None else count
    c.wave = ctypes.cast(rows, ctypes.POINTER(nat.SeaWave))
    return c, rows                                               # (the rows must outlive the call)


def _c_sea(spec):
    c = nat.Sea()
    c.current[:] = spec.current
    c.waves = len(spec.waves)
    for j, w in enumerate(spec.waves):
        c.wave[j] = nat.SeaWave(*w)
    return c


class _Rows:
    """A spectrum the host class would refuse: any rows, unchecked."""

    def __init__(self, current, waves):
        self.current, self.waves = current, list(waves)


def raw_irr(eng, n, state, prev, out, pvo, *, steps=1, step0=0, implicit=0, log=None, applied=None, control=None, mooring=None, layers=3, extremes=None,
            tether=None, net_layers=2, peaks=None):
    """hydro_step_fused_tiled_multi_irr with the guard tests' strides: (rc, rows_written from the sentinel -7)."""
    ptr = lambda b: b.data_ptr() if hasattr(b, "data_ptr") else b  # noqa: E731
    written = ctypes.c_int64(-7)
    rc = eng._lib.hydro_step_fused_tiled_multi_irr(
        eng._h, n, ptr(state), S_IN, ptr(prev), S_PV, DT, steps, ptr(out), S_OUT, ptr(pvo), S_PVO,
        int(implicit), 1, None, ptr(log), 8, 4, 13, 1, 1, 0, ctypes.byref(written),
        ptr(applied), S_A, 0, ptr(control), S_C, ptr(mooring), S_SP3, layers, ptr(extremes), S_E, ptr(tether), S_T2, net_layers,
        ptr(peaks), S_P2, step0, eng._stream(None))
    return rc, written.value


def test_set_refusals_keep_what_was_set_and_a_sea_and_a_spectrum_exclude_each_other(vpop, native_built):
    st = vpop[0]
    n = 65
    eng = _engine(n, vpop[2]["f32"], "f32")
    lib, h, E_ARG, E_STATE = eng._lib, eng._h, -1, -5
    cur = _tiled(st[:n])
    out = eng.alloc_tiled(4, n)
    last = lambda: lib.hydro_last_error(h).decode()  # noqa: E731
    sample = lambda: lib.hydro_sea_spectrum_sample(h, n, cur.data_ptr(), 832, 5, DT, out.data_ptr(), 256, eng._stream(None))  # noqa: E731
    out.fill_(NAN)
    assert sample() == E_STATE and "hydro_set_sea_spectrum" in last()           # no spectrum yet: nothing launched, nothing written
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    c, keep = _c_spectrum(FULL)
    assert lib.hydro_set_sea_spectrum(h, ctypes.byref(c)) == 0 and sample() == 0
    torch.cuda.synchronize()
    before = out.clone()
    assert torch.isfinite(before.permute(0, 2, 1).reshape(-1, 4)[:n]).all() and torch.isnan(before.permute(0, 2, 1).reshape(-1, 4)[n:]).all()
    nan, inf = float("nan"), float("inf")
    good = FULL.waves[0]
    bad = [_c_spectrum(_Rows(FULL.current, list(FULL.waves) + [good])),                     # 65 components
           _c_spectrum(FULL, count=-1), _c_spectrum(_Rows((nan, 0.0, 0.0), [good])), _c_spectrum(_Rows((0.0, 0.0, inf), [good])),
           _c_spectrum(_Rows(FULL.current, [good, (-0.1, 0.06, 0.02, 0.8, 0.3)])), _c_spectrum(_Rows(FULL.current, [(0.1, 0.0, 0.0, 0.8, 0.3)])),
           _c_spectrum(_Rows(FULL.current, list(FULL.waves[:63]) + [(0.1, nan, 0.0, 0.8, 0.0)])),      # the last of 64 is looked at too
           _c_spectrum(_Rows(FULL.current, [(0.1, 0.06, 0.02, inf, 0.0)])), _c_spectrum(_Rows(FULL.current, [(inf, 0.06, 0.02, 0.8, 0.0)]))]
    null_rows, _ = _c_spectrum(FULL)
    null_rows.wave = None                                        # a NULL `wave` with waves > 0
    for c_bad in [b[0] for b in bad] + [null_rows]:
        assert lib.hydro_set_sea_spectrum(h, ctypes.byref(c_bad)) == E_ARG and "sea spectrum" in last()
        out.fill_(NAN)
        assert sample() == 0
        torch.cuda.synchronize()
        assert _same_bits(out, before)                           # the previous spectrum is still in force
    # a sea while a spectrum is set, and the message names the call that clears the spectrum; the spectrum stays
    sea8 = _c_sea(ssr.truncated(FULL, 8))
    assert lib.hydro_set_sea(h, ctypes.byref(sea8)) == E_STATE and "hydro_set_sea_spectrum(h, NULL)" in last()
    assert lib.hydro_sea_sample(h, n, cur.data_ptr(), 832, 5, DT, out.data_ptr(), 256, eng._stream(None)) == E_STATE      # no sea was set by it
    out.fill_(NAN)
    assert sample() == 0
    torch.cuda.synchronize()
    assert _same_bits(out, before)
    assert lib.hydro_set_sea(h, None) == 0                       # clearing is always allowed
    # the other way round
    assert lib.hydro_set_sea_spectrum(h, None) == 0 and sample() == E_STATE
    assert lib.hydro_set_sea(h, ctypes.byref(sea8)) == 0
    assert lib.hydro_set_sea_spectrum(h, ctypes.byref(c)) == E_STATE and "hydro_set_sea(h, NULL)" in last()
    assert sample() == E_STATE and lib.hydro_set_sea_spectrum(h, None) == 0
    assert lib.hydro_sea_sample(h, n, cur.data_ptr(), 832, 5, DT, out.data_ptr(), 256, eng._stream(None)) == 0          # the sea stayed
    assert lib.hydro_set_sea(h, None) == 0 and lib.hydro_set_sea_spectrum(h, ctypes.byref(c)) == 0
    # what is legal at the edges: no components with a NULL wave, 64 components, a component of amplitude 0 without a wave vector
    empty = nat.SeaSpectrum()
    assert lib.hydro_set_sea_spectrum(h, ctypes.byref(empty)) == 0 and lib.hydro_set_sea_spectrum(h, ctypes.byref(c)) == 0
    assert lib.hydro_set_sea_spectrum(h, ctypes.byref(_c_spectrum(_Rows(FULL.current, [(0.0, 0.0, 0.0, 0.0, 0.0)]))[0])) == 0
    # the sample's own refusals
    assert lib.hydro_set_sea_spectrum(h, ctypes.byref(c)) == 0
    out.fill_(NAN)
    for args in ((n, cur.data_ptr(), 832, -1, DT, out.data_ptr(), 256), (n, cur.data_ptr(), 832, 2 ** 52, DT, out.data_ptr(), 256),
                 (n, cur.data_ptr(), 832, 0, 0.0, out.data_ptr(), 256), (n, None, 832, 0, DT, out.data_ptr(), 256),
                 (n, cur.data_ptr(), 832, 0, DT, None, 256), (n, cur.data_ptr(), 832, 0, DT, out.data_ptr(), 255),
                 (n, cur.data_ptr(), 832, 0, DT, out.data_ptr() + 4, 256), (n + 1, cur.data_ptr(), 832, 0, DT, out.data_ptr(), 256)):
        assert lib.hydro_sea_spectrum_sample(h, *args, eng._stream(None)) == E_ARG, args
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    del keep
    eng.close()


def test_step_refusals_launch_nothing(pop, native_built):
    """The spread entry's refusals in its order, with a spectrum set and without one."""
    n = 321
    tiles = (n + 63) // 64
    eng = _engine(n, pop["params"]["f32"], "f32")
    state, prev = _guarded(pop["st"][:n], S_IN), _guarded(pop["pv"][:n], S_PV)
    a, c17 = _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    sp, net = _guarded(pop["spread"][:n, 0:27], S_SP3), _guarded(net_for(pop["net"], n, 2), S_T2)
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    p2 = torch.full((tiles * S_P2,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    call = lambda **kw: raw_irr(eng, n, state, prev, out, pvo, **kw)  # noqa: E731
    for spectrum in (FULL, None):
        eng.set_sea_spectrum(spectrum)
        eng.set_watch(None)
        assert call(step0=-1) == (E_ARG, -7) and call(step0=2 ** 52 - 1) == (E_ARG, -7) and call(steps=3, step0=2 ** 52 - 3) == (E_ARG, -7)
        assert call(steps=0) == (E_ARG, -7)
        assert call(applied=a.data_ptr() + 4) == (E_ARG, -7) and call(control=c17.data_ptr() + 4) == (E_ARG, -7)
        assert call(control=out.data_ptr()) == (E_ARG, -7)                                       # control aliases state_out
        assert call(log=log) == (E_STATE, -7)                                                      # a log without a watch list
        assert call(mooring=sp, layers=0) == (E_ARG, -7) and "mooring_layers" in last()
        assert call(mooring=sp, layers=5) == (E_ARG, -7) and "mooring_layers" in last()
        assert call(mooring=sp, layers=4) == (E_ARG, -7) and "stride" in last()                    # the stride of three layers is below 576 * 4
        assert call(mooring=sp.data_ptr() + 4) == (E_ARG, -7)
        assert call(mooring=sp, extremes=e8.data_ptr() + 4) == (E_ARG, -7)
        assert call(tether=net, net_layers=5) == (E_ARG, -7) and "tether_layers" in last()
        assert call(peaks=p2) == (E_ARG, -7) and "tether_peaks without" in last()
        assert call(mooring=sp, extremes=sp.data_ptr() + 4 * 576) == (E_ARG, -7) and "must not overlap" in last()
        eng.set_watch([0, 320])
        assert call(steps=5, log=log) == (E_ARG, -7)                                               # rows 0 .. 4 of 4
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (out, pvo, log, e8, p2)) and _untouched(sp, _guarded(pop["spread"][:n, 0:27], S_SP3).cpu().numpy())
    # the legal launches next to them: the last step index that exists, layers not looked at without a spread, and a recording one with everything
    eng.set_sea_spectrum(FULL)
    assert call(steps=3, step0=2 ** 52 - 4) == (0, 0) and call(layers=9) == (0, 0)
    assert call(steps=3, log=log, applied=a, control=c17, mooring=sp, extremes=e8, tether=net, peaks=p2) == (0, 3)
    torch.cuda.synchronize()
    state3, rest = _unguard(out, n, 13, S_OUT)
    assert not np.isnan(state3).all() and np.isnan(rest).all() and torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T, state3[[0, 320]], equal_nan=True)
    eng.close()


# ---- 8. guard bands round every output ----------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 65 and 200 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or overwritten - state_out,
    prev_out, the log, the extremes, the link tensions and the sample's out - and the inputs are untouched."""
    st, pv = pop["st"], pop["pv"]
    for n in (65, 200):
        tiles = (n + 63) // 64
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_sea_spectrum(FULL)
        eng.set_seabed(BED)
        eng.set_watch([0, n - 1])
        rec, net = pop["spread"][:n, 0:27], net_for(pop["net"], n, 2)
        state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
        m27, t14 = _guarded(rec, S_SP3), _guarded(net, S_T2)
        empty = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32), (n, 1))
        e8, p2 = _guarded(empty, S_E), _guarded(np.zeros((n, 2), np.float32), S_P2)
        before = [b.cpu().numpy() for b in (state, prev, a, c17, m27, t14)]
        out = torch.full((tiles * S_OUT,), NAN, device=DEV)
        pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
        log = torch.full((4, 13, 8), NAN, device=DEV)
        w = torch.full((tiles * S_W,), NAN, device=DEV)
        eng._check(eng._lib.hydro_sea_spectrum_sample(eng._h, n, state.data_ptr(), S_IN, 11, DT, w.data_ptr(), S_W, eng._stream(None)))
        rc, written = raw_irr(eng, n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, log=log, applied=a, control=c17, mooring=m27,
                              extremes=e8, tether=t14, peaks=p2)
        eng._check(rc)
        torch.cuda.synchronize()
        assert written == 3
        got, rest = _unguard(out, n, 13, S_OUT)
        pv_out, prest = _unguard(pvo, n, 6, S_PVO)
        ext, erest = _unguard(e8, n, 8, S_E)
        peaks, krest = _unguard(p2, n, 2, S_P2)
        water, wrest = _unguard(w, n, 4, S_W)
        assert all(np.isnan(r).all() for r in (rest, prest, erest, krest, wrest)), "a sentinel of an output was overwritten"
        assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
        assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, n - 1]].view(np.uint32))     # the last row is the final state
        assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m27, t14), before))
        assert np.isfinite(water).all() and (np.isfinite(got).all() or not implicit), "a sentinel was read"
        cur, old = _buffers(st, pv, n)
        want_ext, want_peaks = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
        want, want_prev = _launch(eng, "irr", cur, old, n, 3, step0=11, spread=_tiled(rec), layers=3, tether=_tiled(net), net_layers=2, peaks=want_peaks,
                                  extremes=want_ext, control=_tiled(pop["ctl"][:n]), applied=_tiled(pop["applied"][:n]), implicit=implicit)
        torch.cuda.synchronize()
        assert _same(got, _from(want, n)) and _same(pv_out, _from(want_prev, n)) and _same(ext, _from(want_ext, n)) and _same(peaks, _from(want_peaks, n))
        assert _same(water, _from(_sample(eng, st, n, 11), n))
        eng.close()


# ---- 9. ClosedLoopSim and the example ---------------------------------------------------------------------------------------------------
def test_sim_runners_agree_with_a_spectrum_set_and_the_kinds_swap(native_built):
    sc = scenes.scene_c2(n=257)
    sea = jonswap(1.0, 6.0, 30.0, spread="cos2", seed=2, current=(0.3, 0.0, 0.0), g=sc.g)
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(5)), ("resident", lambda s: s.run_resident(5)), ("chunks", lambda s: s.run_resident(5, chunk=2)),
                     ("run", lambda s: s.run(5, graph_steps=32))):
        sim = ClosedLoopSim(sc)
        sim.set_sea(sea)
        go(sim)
        finals[name] = sim.state()
        sim.close()
    assert all(_same(finals["eager"], finals[k]) for k in ("resident", "chunks", "run"))
    plain = ClosedLoopSim(sc)
    plain.run_resident(5)
    assert not np.array_equal(finals["eager"], plain.state())
    # a spectrum of 8 components is the regular sea, in the sim as in the library; and the two kinds swap in the one slot
    eight = ssr.truncated(FULL, 8)
    a, b = ClosedLoopSim(sc), ClosedLoopSim(sc)
    a.set_sea(_as_sea(eight))
    b.set_sea(sea)
    b.set_sea(_as_sea(eight))                                    # a spectrum, then a sea: the spectrum is cleared first
    b.set_sea(eight)                                             # and back
    a.run_resident(5)
    b.run_resident(5)
    assert _same(a.state(), b.state()) and b.engine.spectrum_waves == 8 and b.engine.sea_waves is None
    b.clear_sea()
    assert b.sea is None and b.engine.spectrum_waves is None
    for s in (plain, a, b):
        s.close()


def test_graph_replays_take_a_current_only_spectrum_and_refuse_components(native_built):
    sc = scenes.scene_c2(n=257)
    current = SeaSpectrum((0.4, -0.1, 0.0))
    g, r, same = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    g.set_sea(current)
    r.set_sea(current)
    same.set_sea(SeaState((0.4, -0.1, 0.0)))
    g.run(64, graph_steps=32)
    r.run_resident(64)
    same.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state()) and _same(r.state(), same.state())
    waves = ClosedLoopSim(sc)
    waves.set_sea(ssr.truncated(FULL, 9))
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    for s in (g, r, same, waves):
        s.close()


def test_irregular_sea_design_loads_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "irregular_sea_design_loads.py"), "--steps", "240"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    assert len(re.findall(r"peak tension +([\d.]+) N", res.stdout)) == 9
    m = re.search(r"largest \|device eta - SeaSpectrum.elevation\| = ([\d.e+-]+) m", res.stdout)
    assert m and float(m.group(1)) <= 1e-4, res.stdout
    assert "64 components" in res.stdout
