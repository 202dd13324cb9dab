"""The sea state on the device (hydro_set_sea, hydro_sea_sample, hydro_step_fused_tiled_multi_sea): without a sea the entry
is the pose-hold entry, bit for bit, and so is a sea that does not move; the view (eta, u) follows the fp64 restatement of
tests/sea_reference.py; an explicit step is, bit for bit, the wrench kernel on the relative state followed by the integrator
kernel on the true one, and with implicit drag, applied wrench and pose hold it follows the fp64 step within the project's own
bound; the wave phase advances inside a launch; a released body drifts with the current and a buoy rides the wave; guards,
refusals, ClosedLoopSim, the example.

THE VIEW BOUND.  Errors of hydro_sea_sample against sea_reference.water (fp64), in units of 2^-24 of the scales of
sea_reference.view_scales, over the designed population (coordinates out to 1e4 m: phases of thousands of radians) at step
indices 0, 1, 7 and 10^6.  The bound is the next power of two at or above twice the largest ratio measured on an MI355X:
measured eta 1.66, u 1.77, z_rel 1.65; 2 x 1.77 = 3.54, so VIEW_BOUND = 4 (margin 2.26).  The same fp32 arithmetic emulated on
the host with correctly rounded cos, sin and exp2 gives 1.66 (eta), 1.60 (u): the hardware seeds add next to nothing here.
Bound of the fp64 step comparison: integrator_oracle.STEP_ULP_BOUND (24), scales as in tests/test_pose_hold_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sea_reference as sr
import pose_hold_reference as phr
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import drift_scene, hold_pop, SEA, sea_pop as pop, wave_scene  # noqa: F401  (fixtures are requested by name)
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, G, _guarded, _k, _ke, NAN, raw, _relative,
                              _report, RHO, S_A, S_C, S_IN, S_OUT, S_PV, S_PVO, _same, _same_bits, SIZES, step, STEPS, _tiled, _unguard, _untouched, VIEW_STEPS,
                              _watched)

pytestmark = pytest.mark.gpu
WATCH = (0, 63, 64)                                               # the watched bodies, with the last one
VIEW_BOUND = sr.VIEW_BOUND
S_W = 4 * 64 + 52                                                 # the sample's tile stride in the guard tests


def test_population_meets_the_displaced_surface(pop):
    st, _, params, _, _ = pop
    eta, _ = sr.water(SEA, st[:, 0], st[:, 1], st[:, 2], 0, DT)
    z_rel = st[:, 2] - eta
    ext = scenes.vertical_extent(st[:, 3:7], params["f32"][:, 0:3])
    straddle, submerged = np.abs(z_rel) < ext, z_rel < -ext
    assert straddle.mean() >= 1 / 3 and submerged.mean() >= 1 / 3, (straddle.mean(), submerged.mean())
    assert np.abs(eta).max() > 0.2 and (np.abs(eta) > 0.05).mean() > 0.5          # and the surface IS displaced there


# ---- 1. dispatch and the sea that does not move --------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_no_sea_and_a_still_sea_are_the_pose_hold_entry(coeff, implicit, pop, native_built):
    """No sea set: the bits of hydro_step_fused_tiled_multi_ctl, with and without log, applied and control.  A sea of zero
    current and no waves, and a sea whose one wave has amplitude 0: the same bits - state, prev_out, kinetic energy, log."""
    st, pv, params, applied, ctl = pop
    still = SeaState()
    flat = SeaState().add_wave(0.0, 0.3, -0.2, 1.7, 0.4)
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)
        a, c17 = _tiled(applied[:n]), _tiled(ctl[:n])
        combos = [(steps, app, control, with_log) for steps in STEPS for app in (None, a) for control in (None, c17) for with_log in (False, True)]

        def logs(with_log):
            return dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if with_log else {}
        want = []
        for steps, app, control, with_log in combos:
            cur, old = _buffers(st, pv, n)
            ke, kw = _ke(), logs(with_log)
            eng.step_fused_tiled_multi_controlled(cur, old, n, DT, steps, control, app, "world", implicit_drag=implicit, ke_out=ke, **kw)
            want.append((old, cur[:, 7:13], ke, kw.get("log")))
        for sea in (None, still, flat):
            eng.set_sea(sea)
            for (steps, app, control, with_log), (w_state, w_prev, w_ke, w_log) in zip(combos, want):
                c, o = _buffers(st, pv, n)
                ke, kw = _ke(), logs(with_log)
                got, got_prev = step(eng, "sea", c, o, n, steps, step0=3, control=control, applied=app, implicit=implicit, ke=ke, **kw)
                torch.cuda.synchronize()
                what = (n, steps, app is None, control is None, with_log, None if sea is None else len(sea.waves))
                assert _same_bits(got, w_state) and _same_bits(got_prev, w_prev) and _same_bits(ke, w_ke), what
                assert not with_log or _same_bits(kw["log"], w_log), what
        eng.close()


# ---- 2. the view -------------------------------------------------------------------------------------------------------------------
def test_sample_against_the_fp64_restatement(pop, native_built):
    st, _, params, _, _ = pop
    worst = {"eta": 0.0, "u": 0.0, "z_rel": 0.0}
    for n in SIZES:
        eng = _engine(n, params["f32"], "f32")
        eng.set_sea(SEA)
        cur = _tiled(st[:n])
        s_eta, s_u, s_z = sr.view_scales(SEA, st[:n, 0], st[:n, 1], st[:n, 2])
        for step in VIEW_STEPS:
            got = scenes.from_tiled(eng.sea_sample(cur, n, step, DT).cpu().numpy(), n)
            eta, u = sr.water(SEA, st[:n, 0], st[:n, 1], st[:n, 2], step, DT)
            z_rel = (st[:n, 2] - got[:, 0]).astype(np.float64)                      # the fp32 subtraction the kernel makes
            worst["eta"] = max(worst["eta"], float((np.abs(got[:, 0] - eta) / (sr.ULP * s_eta)).max()))
            worst["u"] = max(worst["u"], float((np.abs(got[:, 1:4] - u) / (sr.ULP * s_u)).max()))
            worst["z_rel"] = max(worst["z_rel"], float((np.abs(z_rel - (st[:n, 2].astype(np.float64) - eta)) / (sr.ULP * s_z)).max()))
            assert np.abs(eta).max() > 0.05 or n == 1
        eng.close()
    print("[sea view] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()) + f"  (bound {VIEW_BOUND:g})")
    assert max(worst.values()) <= VIEW_BOUND, worst


# ---- 3. the step is the existing arithmetic on the relative state ----------------------------------------------------------------------


@COEFFS_SEMANTICS
def test_explicit_step_is_wrench_of_the_relative_state_then_integrator_of_the_true_one(coeff, semantics, pop, native_built):
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea(SEA)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)
        for step0 in (0, 7):
            s_rel, pv_rel = _relative(eng, st, pv, n, step0)
            assert (s_rel[:, 2] != st[:n, 2]).mean() > 0.9 or n == 1
            wrench = eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel))
            cur, old = _buffers(st, pv, n)
            want = eng.integrate_tiled(cur, wrench, n, DT)
            log = torch.full((1, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            got, got_prev = step(eng, "sea", cur, old, n, 1, step0=step0, log=log)
            torch.cuda.synchronize()
            assert _same_bits(got, want), (n, step0)
            assert np.array_equal(got_prev.cpu().numpy().view(np.uint32), scenes.to_tiled(st[:n, 7:13]).view(np.uint32))    # the TRUE velocity
            host = log.cpu().numpy()[0]
            assert np.array_equal(host[:13].T.view(np.uint32), scenes.from_tiled(want.cpu().numpy(), n)[watched].view(np.uint32)), (n, step0)
            assert np.array_equal(host[13:].T.view(np.uint32), scenes.from_tiled(wrench.cpu().numpy(), n)[watched].view(np.uint32)), (n, step0)
        eng.close()


@COEFFS
@DRAG
def test_one_step_with_applied_wrench_and_pose_hold_against_fp64(coeff, implicit, pop, native_built):
    """Reference: integrator_oracle.integrate of the TRUE state with (the device's hydrodynamic wrench of the host-built
    relative state + applied + the pose-hold law of the true state), implicit drag with drag_jacobian of the relative state.
    Bodies within 1e-4 of a branch of the model in the relative state are left out (the oracle quantities drag_jacobian uses
    have branches; the population was gated on the still-water state).  The same comparison with the law evaluated on the
    RELATIVE state (p_z - eta, v - u) must miss the bound: the law is seen to act on the true one."""
    st, pv, params, applied, ctl = pop
    pr = params[coeff]
    worst, wrong = {}, {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(SEA)
        s_rel, pv_rel = _relative(eng, st, pv, n, 7)
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.9 or n == 1, (n, keep.mean())
        hydro = scenes.from_tiled(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)).cpu().numpy(), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step(eng, "sea", cur, old, n, 1, step0=7, control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=implicit)
        torch.cuda.synchronize()
        got = scenes.from_tiled(got.cpu().numpy(), n)
        k = None
        if implicit:
            comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
            k = _k(comps, s_rel, pr, coeff, n)
            k = (k[0][keep], k[1][keep])
        if keep.any():
            worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep])
            # the reference with the law of the relative state instead: hydro + applied + law(s_rel), written as another applied wrench
            swapped = applied[:n].astype(np.float64) + phr.wrench(s_rel, ctl[:n]) - phr.wrench(st[:n], ctl[:n])
            wrong[n] = max(fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=swapped[keep], ctl=ctl[:n][keep]).values())
        eng.close()
    _report(f"sea + applied + pose hold {'implicit' if implicit else 'explicit'} {coeff}", worst)
    assert wrong[max(SIZES)] > 10 * B, wrong


# ---- 4. time advances inside the launch --------------------------------------------------------------------------------------------
@COEFFS
@DRAG
@pytest.mark.parametrize("start", [0, 10 ** 6])
def test_one_launch_equals_single_steps_and_chunks_and_differs_from_a_frozen_phase(coeff, implicit, start, pop, native_built):
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        watched = _watched(n, WATCH)
        eng.set_watch(watched)

        def run(chunks, frozen=False):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 13, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                step(eng, "sea", cur, old, n, k, step0=start if frozen else start + done, implicit=implicit, log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, old[:, 7:13], log
        one, singles, chunks, frozen = run([7]), run([1] * 7), run([2, 5]), run([1] * 7, frozen=True)
        for other in (singles, chunks):
            assert all(_same_bits(x, y) for x, y in zip(one, other)), (n, start)
        finite = torch.isfinite(one[0]).all(dim=1, keepdim=True) & torch.isfinite(frozen[0]).all(dim=1, keepdim=True)
        # a view evaluated once per launch would give `frozen`: the same first step, then apart (n = 1: its one light body may
        # leave the fp32 range within seven explicit steps)
        assert _same_bits(one[2][0], frozen[2][0]) and (n == 1 or not _same_bits(one[2][1], frozen[2][1])), (n, start)
        assert n == 1 or bool(((one[0] != frozen[0]) & finite).any()), (n, start)
        eng.close()


# ---- 5. physics on the device --------------------------------------------------------------------------------------------------------
def _copies(state, prev, params, n=64):
    """n copies of a one-body scene, spread over x and y."""
    st, pv, pr = np.repeat(state, n, 0), np.repeat(prev, n, 0), np.repeat(params, n, 0)
    st[:, 0], st[:, 1] = 7.0 * (np.arange(n) % 8), -11.0 * (np.arange(n) // 8)
    return st, pv, pr


@DRAG
def test_released_bodies_drift_with_the_current(implicit, native_built):
    st, pv, pr, sea = drift_scene()
    st, pv, pr = _copies(st, pv, pr)
    sim = ClosedLoopSim(scenes.Scene("drift", st, pv, pr), implicit_drag=implicit)
    sim.set_sea(sea)
    sim.run_resident(1200, chunk=64)                             # 18 launches of 64 steps and one of 48
    v, U = sim.state()[:, 7:10].astype(np.float64), np.asarray(sea.current)
    drift = np.linalg.norm(v - U, axis=1) / np.linalg.norm(U)
    print(f"[drift on the device, {'implicit' if implicit else 'explicit'}] |v - U| / |U| after 1 200 steps: {drift.min():.3e} .. {drift.max():.3e} (fp64 model: 7.3e-3)")
    assert sim.steps_done == 1200 and drift.max() < 1e-2
    sim.close()


def test_buoys_ride_the_wave(native_built):
    sc, sea, z_eq = wave_scene()
    st, pv, pr = _copies(sc.state, sc.prev, sc.params)
    sim = ClosedLoopSim(scenes.Scene("wave", st, pv, pr, dt=sc.dt))
    sim.set_sea(sea)
    rec = sim.record(list(range(64)), every=1, rows=1920)
    sim.run_resident(1920, chunk=64)
    s = rec.states().astype(np.float64)                          # (1920, 64, 13)
    t = (rec.steps() * sc.dt)[:, None]
    dev = np.abs(s[:, :, 2] - z_eq - sea.elevation(s[:, :, 0], s[:, :, 1], t))
    print(f"[wave on the device] largest |z - z_eq - eta| after step 480: {dev[480:].max():.4f} m (fp64 model, one buoy at the origin: see tests/test_sea.py)")
    assert dev[480:].max() < 0.1
    assert np.ptp(s[600, :, 2]) > 0.05                           # the copies sit at different phases of the wave
    sim.close()


# ---- 6. guards and refusals through the raw C ABI -----------------------------------------------------------------------------------
def _c_sea(current=(0.5, -0.2, 0.05), waves=((0.2, 0.06, 0.02, 0.8, 0.3),), count=None):
    c = nat.Sea()
    c.current[:] = current
    c.waves = len(waves) if count is None else count
    for j, w in enumerate(waves[:nat.SEA_WAVES_MAX]):
        c.wave[j] = nat.SeaWave(*w)
    return c


def test_set_sea_refusals_keep_the_previous_sea(pop, native_built):
    st, _, params, _, _ = pop
    n = 65
    eng = _engine(n, params["f32"], "f32")
    lib, E_ARG, E_STATE = eng._lib, -1, -5
    cur = _tiled(st[:n])
    out = eng.alloc_tiled(4, n)
    sample = lambda: lib.hydro_sea_sample(eng._h, n, cur.data_ptr(), 832, 5, DT, out.data_ptr(), 256, eng._stream(None))  # noqa: E731
    assert sample() == E_STATE                                   # no sea yet
    good = (0.2, 0.06, 0.02, 0.8, 0.3)
    out.fill_(NAN)                                               # the lanes past n are never written: same fill before every sample
    assert lib.hydro_set_sea(eng._h, ctypes.byref(_c_sea())) == 0 and sample() == 0
    torch.cuda.synchronize()
    before = out.clone()
    live = before.permute(0, 2, 1).reshape(-1, 4)[:n]
    assert torch.isfinite(live).all() and (live[:, 0] != 0).any()
    assert torch.isnan(before.permute(0, 2, 1).reshape(-1, 4)[n:]).all()
    nan, inf = float("nan"), float("inf")
    bad = [_c_sea(waves=(good,) * 8, count=9), _c_sea(count=-1), _c_sea(current=(nan, 0.0, 0.0)), _c_sea(current=(0.0, 0.0, inf)),
           _c_sea(waves=((-0.1, 0.06, 0.02, 0.8, 0.3),)), _c_sea(waves=((0.1, 0.0, 0.0, 0.8, 0.3),)), _c_sea(waves=(good, (0.1, nan, 0.0, 0.8, 0.0))),
           _c_sea(waves=((0.1, 0.06, 0.02, inf, 0.0),)), _c_sea(waves=((0.1, 0.06, 0.02, 0.8, nan),)), _c_sea(waves=((inf, 0.06, 0.02, 0.8, 0.0),))]
    for c in bad:
        assert lib.hydro_set_sea(eng._h, ctypes.byref(c)) == E_ARG
        out.fill_(NAN)
        assert sample() == 0
        torch.cuda.synchronize()
        assert _same_bits(out, before)                           # the previous sea is still in force
    # what is legal at the edges: eight components, a wave of amplitude 0 without a wave vector
    assert lib.hydro_set_sea(eng._h, ctypes.byref(_c_sea(waves=(good,) * 8))) == 0
    assert lib.hydro_set_sea(eng._h, ctypes.byref(_c_sea(waves=((0.0, 0.0, 0.0, 0.0, 0.0),)))) == 0
    # the sample's own refusals
    for args in ((n, cur.data_ptr(), 832, -1, DT, out.data_ptr(), 256), (n, cur.data_ptr(), 832, 2 ** 52, DT, out.data_ptr(), 256),
                 (n, cur.data_ptr(), 832, 0, 0.0, out.data_ptr(), 256), (n, None, 832, 0, DT, out.data_ptr(), 256),
                 (n, cur.data_ptr(), 832, 0, DT, None, 256), (n, cur.data_ptr(), 832, 0, DT, out.data_ptr(), 255),
                 (n, cur.data_ptr(), 832, 0, DT, out.data_ptr() + 4, 256), (n + 1, cur.data_ptr(), 832, 0, DT, out.data_ptr(), 256)):
        assert lib.hydro_sea_sample(eng._h, *args, eng._stream(None)) == E_ARG, args
    assert lib.hydro_set_sea(eng._h, None) == 0 and sample() == E_STATE
    eng.close()


def test_step_refusals_launch_nothing(pop, native_built):
    st, pv, params, applied, ctl = pop
    n = 257
    eng = _engine(n, params["f32"], "f32")
    eng.set_sea(SEA)
    tiles = (n + 63) // 64
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    assert raw(eng, "sea", n, state, prev, out, pvo, step0=-1) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, step0=2 ** 52 - 1) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=3, step0=2 ** 52 - 3) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=0) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, applied=a.data_ptr() + 4) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, control=c17.data_ptr() + 4) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, control=out.data_ptr()) == (E_ARG, -7)            # control aliases state_out
    assert raw(eng, "sea", n, state, prev, out, pvo, log=log) == (E_STATE, -7)                         # a log without a watch list
    eng.set_watch([0, 256])
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=5, log=log) == (E_ARG, -7)                  # rows 0 .. 4 of 4
    eng.set_sea(None)                                            # and without a sea the refusals are the pose-hold entry's
    assert raw(eng, "sea", n, state, prev, out, pvo, step0=-1) == (E_ARG, -7)
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=5, log=log) == (E_ARG, -7)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all()
    # the legal launches next to them: the last step index that exists, and a recording one
    eng.set_sea(SEA)
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=3, step0=2 ** 52 - 4) == (0, 0)
    assert raw(eng, "sea", n, state, prev, out, pvo, steps=3, log=log, applied=a.data_ptr(), control=c17.data_ptr()) == (0, 3)
    torch.cuda.synchronize()
    state3, rest = _unguard(out, n, 13, S_OUT)
    assert not np.isnan(state3).all() and np.isnan(rest).all() and torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T, state3[[0, 256]], equal_nan=True)
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 65 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or overwritten - state_out,
    prev_out, log and the sample's out - and the inputs are untouched."""
    st, pv, params, applied, ctl = pop
    n, tiles = 65, 2
    eng = _engine(n, params[coeff], coeff)
    eng.set_sea(SEA)
    eng.set_watch([0, 64])
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
    before = [b.cpu().numpy() for b in (state, prev, a, c17)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    eng._check(eng._lib.hydro_sea_sample(eng._h, n, state.data_ptr(), S_IN, 11, DT, w.data_ptr(), S_W, eng._stream(None)))
    rc, written = raw(eng, "sea", n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, log=log, applied=a.data_ptr(), control=c17.data_ptr())
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    water, wrest = _unguard(w, n, 4, S_W)
    assert np.isnan(rest).all() and np.isnan(prest).all() and np.isnan(wrest).all(), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 64]].view(np.uint32))      # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17), before))
    assert np.isfinite(water).all(), "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want, want_prev = step(eng, "sea", cur, old, n, 3, step0=11, control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint32), scenes.from_tiled(want.cpu().numpy(), n).view(np.uint32))
    assert np.array_equal(pv_out.view(np.uint32), scenes.from_tiled(want_prev.contiguous().cpu().numpy(), n).view(np.uint32))
    assert np.array_equal(water.view(np.uint32), scenes.from_tiled(eng.sea_sample(_tiled(st[:n]), n, 11, DT).cpu().numpy(), n).view(np.uint32))
    eng.close()


# ---- 7. ClosedLoopSim and the example ---------------------------------------------------------------------------------------------------
def _c2():
    return scenes.scene_c2(n=257)


def test_sim_runners_agree_with_a_sea_set(native_built):
    sc = _c2()
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(5)), ("resident", lambda s: s.run_resident(5)), ("chunks", lambda s: s.run_resident(5, chunk=2))):
        sim = ClosedLoopSim(sc)
        sim.set_sea(SEA)
        go(sim)
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc)
    plain.run_resident(5)
    assert _same(finals["eager"], finals["resident"]) and _same(finals["eager"], finals["chunks"])
    assert not np.array_equal(finals["eager"], plain.state())
    plain.close()


def test_graph_replays_with_a_current_and_clear_sea(native_built):
    sc = _c2()
    current = SeaState((0.4, -0.1, 0.0))
    g, r, never, cleared = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    g.set_sea(current)
    r.set_sea(current)
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state())
    never.run_resident(64)
    assert not np.array_equal(r.state(), never.state())
    cleared.set_sea(SEA)
    cleared.clear_sea()
    assert cleared.sea is None
    cleared.run_resident(32)
    cleared.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state())
    waves = ClosedLoopSim(sc)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_sea(current)
    for s in (g, r, never, cleared, waves, two_kernel):
        s.close()


def test_buoy_in_waves_example(tmp_path, native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "buoy_in_waves.py"), "--steps", "600", "--chunk", "200", "--out", str(tmp_path)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    m = re.search(r"largest \|z - z_eq - eta\| over 600 steps \([\d.]+ s\): ([\d.]+) m", res.stdout)
    assert m and float(m.group(1)) < 0.1, res.stdout
    rows = open(os.path.join(tmp_path, "velocity_log.csv")).read().strip().splitlines()
    assert len(rows) == 601                                      # the header and one row per step
