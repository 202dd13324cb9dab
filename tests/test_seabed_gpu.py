"""The seabed on the device (hydro_set_seabed, hydro_seabed_wrench, hydro_step_fused_tiled_multi_bed): without a bed, and with
a bed nobody reaches, the entry is the sea entry bit for bit; the probe follows the fp64 restatement of
tests/seabed_reference.py; a bed step is, bit for bit, the sea entry's step given the probe's wrench as a world-frame applied
wrench; with implicit drag, applied wrench, pose hold and sea it follows the fp64 step within the project's own bound - and
misses it if the bed is given the sea-relative state; a launch of 7 steps equals 7 of 1 and (2, 5); the CPU test's boxes come
to rest on the device; guards, refusals, ClosedLoopSim's three runners, the example.

Sizes: n = 200 (one block: three full tiles and 8 lanes) and n = 321 (two blocks, the last wave with one live lane).

THE PROBE BOUND.  Errors of hydro_seabed_wrench against seabed_reference.wrench (fp64, with the kernel's own decision which
corners are below the plane: seabed_reference.touching_fp32), in units of 2^-24 of seabed_reference.wrench_scales, over the
designed population.  The rule: the next power of two at or above twice the largest ratio measured on an MI355X.  NO DEVICE
FIGURE YET: this file has not run on an MI355X.  PROBE_BOUND = 4 stands on the same
arithmetic emulated on the host in fp32 over this population (seabed_reference.wrench_fp32_emulated: the header's order, a
correctly rounded seed for the reciprocal square root): force 1.98, torque 0.76; 2 x 1.98 = 3.97.  The test prints the
device's figures; the first run on an MI355X is to replace these two and, if twice its largest exceeds 4, the bound.
Bound of the fp64 step comparison: integrator_oracle.STEP_ULP_BOUND (24), scales as in tests/test_pose_hold_gpu.py with the
bed's own term magnitudes (seabed_reference.wrench_scales) added to the surrogate wrench."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seabed_reference as br
import sea_reference as sr
from conftest import REPO
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import (ALL_TILE, BED, bed_pop as pop, FAR, hold_pop, _lowest_fp32, NEAR, NONE_TILE, rest_report, REST_V, REST_W, REST_Z, SEA,
                                  settling_boxes, SIZES, STEPS, Z_B, Z_BED)  # noqa: F401  (fixtures are requested by name)
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, NAN, raw, RHO, S_A,
                              S_C, S_IN, S_OUT, S_PV, S_PVO, _same, _same_bits, step, _tiled, _unguard, _untouched, _watched)
from seabed_reference import PROBE_BOUND

pytestmark = pytest.mark.gpu
S_W = 6 * 64 + 28                                                 # the probe's tile stride in the guard tests


def test_population_meets_the_bed(pop):
    st, _, params, _, _ = pop
    pr = params["f32"]
    for touch in (None, br.touching_fp32(BED, st, pr)):          # decided in fp64, and as the kernel decides
        count = br.corner_count(BED, st, pr, touch)
        for n in SIZES:
            c = count[:n]
            assert ((c >= 1) & (c <= 3)).mean() >= 0.25 and (c >= 4).mean() >= 0.25 and (c == 0).mean() >= 0.25, (n, np.bincount(c, minlength=9))
        assert (count[64 * NONE_TILE:64 * NONE_TILE + 64] == 0).all() and (count[64 * ALL_TILE:64 * ALL_TILE + 64] >= 1).all()
        assert count[320] >= 4
    low, _ = _lowest_fp32(st[NEAR], pr[NEAR])
    ulps = (low.astype(np.float64) - Z_BED) / np.spacing(np.float32(abs(Z_BED)))
    assert sorted(ulps.tolist()) == [-1, -1, -1, 0, 0, 0, 1, 1]
    fp32 = br.touching_fp32(BED, st[NEAR], pr[NEAR]).sum(axis=1)
    assert ((fp32 >= 1) == (ulps < 0)).all()                     # below the plane touches; on it and above it does not
    q = np.linalg.norm(st[:, 3:7].astype(np.float64), axis=1)
    assert (np.abs(q - 1) > 5e-4).sum() >= 8 and (np.abs(st[:, 7:13]) > 0).any(axis=1).mean() > 0.9
    assert not (br.corner_count(FAR, st, pr) > 0).any()


# ---- 1. no bed, and a bed nobody reaches -----------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_no_bed_and_a_far_bed_are_the_sea_entry(coeff, implicit, pop, native_built):
    """No bed set, and a bed at z_b = -1e6: the bits of hydro_step_fused_tiled_multi_sea - state, prev_out, kinetic energy and
    the recorded state and wrench - with and without log, applied wrench, control and sea."""
    st, pv, params, applied, ctl = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        watched = _watched(n)
        eng.set_watch(watched)
        a, c17 = _tiled(applied[:n]), _tiled(ctl[:n])
        combos = [(steps, app, control, with_log) for steps in STEPS for app in (None, a) for control in (None, c17) for with_log in (False, True)]

        def logs(with_log):
            return dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if with_log else {}
        for sea in (None, SEA):
            eng.set_sea(sea)
            eng.set_seabed(None)
            want = []
            for steps, app, control, with_log in combos:
                cur, old = _buffers(st, pv, n)
                ke, kw = _ke(), logs(with_log)
                state, prev = step(eng, "sea", cur, old, n, steps, step0=3, control=control, applied=app, implicit=implicit, ke=ke, **kw)
                want.append((state, prev, ke, kw.get("log")))
            for bed in (None, FAR):
                eng.set_seabed(bed)
                for (steps, app, control, with_log), (w_state, w_prev, w_ke, w_log) in zip(combos, want):
                    c, o = _buffers(st, pv, n)
                    ke, kw = _ke(), logs(with_log)
                    got, got_prev = step(eng, "bed", c, o, n, steps, step0=3, control=control, applied=app, implicit=implicit, ke=ke, **kw)
                    torch.cuda.synchronize()
                    what = (n, steps, app is None, control is None, with_log, sea is None, bed is None)
                    assert _same_bits(got, w_state) and _same_bits(got_prev, w_prev) and _same_bits(ke, w_ke), what
                    assert not with_log or _same_bits(kw["log"], w_log), what
        eng.close()


# ---- 2. the probe ------------------------------------------------------------------------------------------------------------------
@COEFFS
def test_probe_against_the_fp64_restatement(coeff, pop, native_built):
    st, _, params, _, _ = pop
    pr = params[coeff]
    worst = {"force": 0.0, "torque": 0.0}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_seabed(BED)
        got = _from(eng.seabed_wrench(_tiled(st[:n]), n), n)
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        ref, scale = br.wrench(BED, st[:n], pr[:n], touch), br.wrench_scales(BED, st[:n], pr[:n], touch)
        none = ~touch.any(axis=1)
        assert not got[none].any() and not np.signbit(got[none]).any() and none.sum() >= n // 4          # +0 where nothing touches
        assert np.isfinite(got).all() and (got[~none, 2] >= 0).all() and (got[~none, 2] > 0).mean() > 0.8
        flat = scale == 0                                        # (a body at rest: no term forms its friction, and there is none)
        assert not got[flat].any() and not ref[flat].any()
        err = np.abs(got[~none] - ref[~none]) / (br.ULP * np.where(flat, 1.0, scale)[~none])
        worst["force"] = max(worst["force"], float(err[:, 0:3].max()))
        worst["torque"] = max(worst["torque"], float(err[:, 3:6].max()))
        eng.close()
    print(f"[seabed probe, {coeff}] largest error in units of 2^-24 of the scale: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"  (bound {PROBE_BOUND:g})")
    assert max(worst.values()) <= PROBE_BOUND, worst


# ---- 3. a bed step is the sea entry's step with the probe's wrench applied ---------------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
@pytest.mark.parametrize("moving", [False, True], ids=["still", "sea"])
def test_bed_step_is_the_sea_step_with_the_probe_wrench_applied(coeff, semantics, implicit, moving, pop, native_built):
    st, pv, params, _, _ = pop
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1]) if moving else None
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_seabed(BED)
        eng.set_sea(sea)
        watched = _watched(n)
        eng.set_watch(watched)
        probe = eng.seabed_wrench(_tiled(st[:n]), n)
        assert (_from(probe, n)[:, 2] > 0).mean() > 0.5
        logs = [torch.full((1, 19, len(watched)), NAN, dtype=torch.float32, device=DEV) for _ in range(2)]
        cur, old = _buffers(st, pv, n)
        want, want_prev = step(eng, "sea", cur, old, n, 1, step0=7, applied=probe, implicit=implicit, log=logs[0])
        cur, old = _buffers(st, pv, n)
        got, got_prev = step(eng, "bed", cur, old, n, 1, step0=7, implicit=implicit, log=logs[1])
        torch.cuda.synchronize()
        assert _same_bits(got, want) and _same_bits(got_prev, want_prev), n
        assert _same_bits(logs[1], logs[0]), n                   # the recorded state and the recorded wrench
        touching = (_from(probe, n)[watched] != 0).any(axis=1)
        assert touching.any() and not touching.all()
        eng.close()


# ---- 4. everything together against fp64 ---------------------------------------------------------------------------------------------


@COEFFS
def test_one_step_with_everything_against_fp64(coeff, pop, native_built):
    """Implicit drag + applied wrench + pose hold + sea + bed.  Reference: integrator_oracle.integrate of the TRUE state with
    (the device's hydrodynamic wrench of the host-built relative state + applied + the pose-hold law + the fp64 bed wrench of
    the TRUE state, corners decided as the kernel decides them), drag_jacobian of the relative state.  Bodies within 1e-4 of a
    branch of the hydrodynamic model in the relative state are left out, as in tests/test_sea_gpu.py.  The same reference
    with the bed evaluated on the sea-RELATIVE state must miss by more than ten bounds."""
    st, pv, params, applied, ctl = pop
    pr = params[coeff]
    worst, wrong = {}, {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        w = _from(eng.sea_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = step(eng, "bed", cur, old, n, 1, step0=7, control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        comps = ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2]
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
        touch = br.touching_fp32(BED, st[:n], pr[:n])
        bed_w, bed_s = br.wrench(BED, st[:n], pr[:n], touch), br.wrench_scales(BED, st[:n], pr[:n], touch)
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=bed_w[keep], bed_scale=bed_s[keep])
        rel_w = br.wrench(BED, s_rel, pr[:n])
        wrong[n] = max(fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=applied[:n][keep], ctl=ctl[:n][keep], bed_wrench=rel_w[keep], bed_scale=bed_s[keep]).values())
        eng.close()
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[sea + applied + pose hold + bed, implicit, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g}); with the bed on the relative state: {min(wrong.values()):.0f}")
    assert max(per_group.values()) <= B, worst
    assert min(wrong.values()) > 10 * B, wrong


# ---- 5. step counts ------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        watched = _watched(n)
        eng.set_watch(watched)

        def run(chunks):
            cur, old = _buffers(st, pv, n)
            log = torch.full((7, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            done = 0
            for k in chunks:
                step(eng, "bed", cur, old, n, k, step0=100 + done, implicit=implicit, log=log, every=1, phase=1, row0=done)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, old[:, 7:13], log
        one, singles, chunks = run([7]), run([1] * 7), run([2, 5])
        for other in (singles, chunks):
            assert all(_same_bits(x, y) for x, y in zip(one, other)), n
        assert not torch.isnan(one[2][0]).any()
        eng.close()


# ---- 6. the boxes come to rest on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [60, 120])
def test_boxes_come_to_rest_on_the_device(rate, native_built):
    st, pv, pr, ratios = settling_boxes()
    reps = -(-64 // len(st))
    st, pv, pr, ratios = (np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:64] for a in (st, pv, pr, ratios))
    st[:, 0], st[:, 1] = 3.0 * (np.arange(64) % 8), -3.0 * (np.arange(64) // 8)
    dt = float(np.float32(1.0 / rate))
    bed = Seabed.for_step(Z_B, dt)
    sim = ClosedLoopSim(scenes.Scene("boxes", st, pv, pr, dt=dt), implicit_drag=True)
    sim.set_seabed(bed)
    sim.run_resident(12 * rate, chunk=64)
    contacts, v, w, off = rest_report(bed, sim.state(), pr, ratios)
    print(f"[rest on the device, dt = 1/{rate}] corners {sorted(set(contacts.tolist()))}  |v| <= {v.max():.2e} m/s  |omega| <= {w.max():.2e} rad/s  "
          f"lowest corner off the analytic depth by <= {off.max():.2e} m")
    assert sim.steps_done == 12 * rate and (contacts == 4).all(), contacts
    assert v.max() < REST_V and w.max() < REST_W and off.max() < REST_Z, (v.max(), w.max(), off.max())
    sim.close()


# ---- 7. refusals and guards through the raw C ABI ------------------------------------------------------------------------------------
def _c_bed(z=-3.0, stiffness=144.0, damping=2.4, friction=0.5, slip_speed=0.01, friction_rate=2.4):
    return nat.Seabed(z, stiffness, damping, friction, slip_speed, friction_rate)


def test_set_seabed_refusals_keep_the_previous_bed(pop, native_built):
    st, _, params, _, _ = pop
    n = 200
    eng = _engine(n, params["f32"], "f32")
    lib, E_ARG, E_STATE = eng._lib, -1, -5
    cur = _tiled(st[:n])
    out = eng.alloc_tiled(6, n)
    probe = lambda: lib.hydro_seabed_wrench(eng._h, n, cur.data_ptr(), 832, out.data_ptr(), 384, eng._stream(None))  # noqa: E731
    assert probe() == E_STATE                                    # no bed yet
    out.fill_(NAN)
    assert lib.hydro_set_seabed(eng._h, ctypes.byref(_c_bed())) == 0 and probe() == 0
    torch.cuda.synchronize()
    before = out.clone()
    live = before.permute(0, 2, 1).reshape(-1, 6)[:n]
    assert torch.isfinite(live).all() and (live[:, 2] > 0).any()
    assert torch.isnan(before.permute(0, 2, 1).reshape(-1, 6)[n:]).all()
    nan, inf = float("nan"), float("inf")
    bad = [dict(z=nan), dict(z=inf), dict(z=-inf), dict(z=1e39), dict(stiffness=nan), dict(stiffness=-1.0), dict(stiffness=inf), dict(stiffness=1e39),
           dict(damping=nan), dict(damping=-1e-9), dict(damping=1e39), dict(friction=nan), dict(friction=-0.5), dict(friction=inf),
           dict(slip_speed=0.0), dict(slip_speed=-0.01), dict(slip_speed=nan), dict(slip_speed=inf), dict(slip_speed=1e-30), dict(slip_speed=1e30),
           dict(friction_rate=nan), dict(friction_rate=-2.4), dict(friction_rate=1e39)]
    for kw in bad:
        assert lib.hydro_set_seabed(eng._h, ctypes.byref(_c_bed(**kw))) == E_ARG, kw
        out.fill_(NAN)
        assert probe() == 0
        torch.cuda.synchronize()
        assert _same_bits(out, before), kw                       # the previous bed is still in force
    # what is legal at the edges: a plane above the surface, no spring, no damper, no friction, no cap
    assert lib.hydro_set_seabed(eng._h, ctypes.byref(_c_bed(z=2.0, stiffness=0.0, damping=0.0, friction=0.0, friction_rate=0.0))) == 0
    # the probe's own refusals
    for args in ((n, None, 832, out.data_ptr(), 384), (n, cur.data_ptr(), 832, None, 384), (n, cur.data_ptr(), 832, out.data_ptr(), 383),
                 (n, cur.data_ptr(), 832, out.data_ptr() + 4, 384), (n, cur.data_ptr(), 831, out.data_ptr(), 384),
                 (n + 1, cur.data_ptr(), 832, out.data_ptr(), 384), (-1, cur.data_ptr(), 832, out.data_ptr(), 384)):
        assert lib.hydro_seabed_wrench(eng._h, *args, eng._stream(None)) == E_ARG, args
    assert lib.hydro_set_seabed(eng._h, None) == 0 and probe() == E_STATE
    eng.close()


def test_step_refusals_launch_nothing(pop, native_built):
    """The refusals are the sea entry's, in its order, with a bed set and without; the bed adds none."""
    st, pv, params, applied, ctl = pop
    n = 321
    eng = _engine(n, params["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    for bed, sea in ((BED, None), (BED, SEA), (None, None)):
        eng.set_watch(None)
        eng.set_seabed(bed)
        eng.set_sea(sea)
        assert raw(eng, "bed", n, state, prev, out, pvo, step0=-1) == (E_ARG, -7)
        assert raw(eng, "bed", n, state, prev, out, pvo, step0=2 ** 52 - 1) == (E_ARG, -7)
        assert raw(eng, "bed", n, state, prev, out, pvo, steps=0) == (E_ARG, -7)
        assert raw(eng, "bed", n, state, prev, out, pvo, applied=a.data_ptr() + 4) == (E_ARG, -7)
        assert raw(eng, "bed", n, state, prev, out, pvo, control=c17.data_ptr() + 4) == (E_ARG, -7)
        assert raw(eng, "bed", n, state, prev, out, pvo, control=out.data_ptr()) == (E_ARG, -7)        # control aliases state_out
        assert raw(eng, "bed", n, state, prev, out, pvo, log=log) == (E_STATE, -7)                     # a log without a watch list
        eng.set_watch([0, 320])
        assert raw(eng, "bed", n, state, prev, out, pvo, steps=5, log=log) == (E_ARG, -7)              # rows 0 .. 4 of 4
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all()
    eng.close()


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200 with tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n
    of every buffer: the bodies' outputs are those of the tightly packed launch, no sentinel is read or overwritten - state_out,
    prev_out, log and the probe's out - and the inputs are untouched."""
    st, pv, params, applied, ctl = pop
    n, tiles = 200, 4
    eng = _engine(n, params[coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
    before = [b.cpu().numpy() for b in (state, prev, a, c17)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    w = torch.full((tiles * S_W,), NAN, device=DEV)
    eng._check(eng._lib.hydro_seabed_wrench(eng._h, n, state.data_ptr(), S_IN, w.data_ptr(), S_W, eng._stream(None)))
    rc, written = raw(eng, "bed", n, state, prev, out, pvo, steps=3, step0=11, implicit=implicit, log=log, applied=a.data_ptr(), control=c17.data_ptr())
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == 3
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    contact, wrest = _unguard(w, n, 6, S_W)
    assert np.isnan(rest).all() and np.isnan(prest).all() and np.isnan(wrest).all(), "a sentinel of an output was overwritten"
    assert torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17), before))
    assert np.isfinite(contact).all(), "a sentinel was read"
    cur, old = _buffers(st, pv, n)
    want, want_prev = step(eng, "bed", cur, old, n, 3, step0=11, control=_tiled(ctl[:n]), applied=_tiled(applied[:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint32), _from(want, n).view(np.uint32))
    assert np.array_equal(pv_out.view(np.uint32), _from(want_prev, n).view(np.uint32))
    assert np.array_equal(contact.view(np.uint32), _from(eng.seabed_wrench(_tiled(st[:n]), n), n).view(np.uint32))
    eng.close()


# ---- 8. ClosedLoopSim and the example ---------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 321) sunk to just above a bed at z = -3 m, as dense as rock: most of them land within the run."""
    sc = scenes.scene_c2(n=321)
    st, pr = sc.state.copy(), sc.params.copy()
    st[:, 2] = Z_BED + 0.5 * np.linalg.norm(pr[:, 0:3], axis=1) + 0.01
    pr[:, 10] = 2.5 * sc.rho * pr[:, 0:3].prod(axis=1)
    return scenes.Scene("c2 on the bed", st, sc.prev, pr, dt=sc.dt)


def test_sim_runners_agree_with_a_bed_set(native_built):
    sc = _scene()
    bed = Seabed.for_step(Z_BED, sc.dt)
    finals = {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.set_seabed(bed)
        go(sim)
        assert name != "graph" or sim._graph is not None
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc, implicit_drag=True)
    plain.run_resident(64)
    for name in ("resident", "chunks", "graph"):
        assert _same(finals["eager"], finals[name]), name
    fell = plain.state()
    assert (finals["eager"][:, 2] > fell[:, 2] + 1e-3).mean() > 0.5               # the bed held most of them up
    plain.close()


def test_graph_replays_with_bed_and_current_and_clear_seabed(native_built):
    sc = _scene()
    bed, current = Seabed.for_step(Z_BED, sc.dt), SeaState((0.4, -0.1, 0.0))
    g, r, never, cleared = (ClosedLoopSim(sc, implicit_drag=True) for _ in range(4))
    for s in (g, r):
        s.set_sea(current)
        s.set_seabed(bed)
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and _same(g.state(), r.state())
    never.run_resident(64)
    assert not np.array_equal(r.state(), never.state())
    cleared.set_seabed(bed)
    cleared.clear_seabed()
    assert cleared.seabed is None
    cleared.run_resident(32)
    cleared.run(32, graph_steps=32)
    assert _same(cleared.state(), never.state())
    waves = ClosedLoopSim(sc, implicit_drag=True)
    waves.set_seabed(bed)
    waves.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_seabed(bed)
    for s in (g, r, never, cleared, waves, two_kernel):
        s.close()


def test_boxes_on_seabed_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "boxes_on_seabed.py"), "--boxes", "256", "--steps", "720", "--chunk", "240"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    m = re.search(r"at rest on four corners: (\d+) of 256", res.stdout)
    assert m and int(m.group(1)) == 256, res.stdout
    m = re.search(r"rest depth against g \(1 - rho / rho_body\) / \(4 kappa\): largest difference ([\d.e+-]+) m", res.stdout)
    assert m and float(m.group(1)) < 1e-4, res.stdout
