"""The pose hold on the device (hydro_step_fused_tiled_multi_ctl): without a control record the entry is the applied entry,
bit for bit; zero gains change nothing; one step follows the fp64 step within the project's own bound; the law acts in every
step of a launch (a resident launch equals single stepping and differs from a zero-order hold); directions and the clamp by
hand on dry bodies; the recorder logs the total wrench; guards, refusals, ClosedLoopSim, the example.

Bound of the fp64 comparisons: integrator_oracle.STEP_ULP_BOUND (24).  The reference is integrator_oracle.integrate of (the
device's fp32 hydrodynamic wrench + the applied wrench + the law of tests/pose_hold_reference.py), all sums in fp64.  The
scales are those of field_scales on a surrogate wrench that extends the applied test's by the sizes of the law's terms
before they cancel: per axis |F_hydro,i| + |f_applied| + |(|kp e_p| + |kd v|)|, and |tau_hydro| + |tau_applied| +
kp_ang 2 |q*| |q| + kd_ang |omega|.  Each of those tests prints its largest error per group.
Measured on an MI355X: see DESIGN.md section 16."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pose_hold_reference as phr
from conftest import REPO
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.simulate import ClosedLoopSim, recorder_cadence
from designed_populations import hold_pop as pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import (B, _bits, _buffers, COEFFS, DEV, DRAG, DT, _engine, fp64_step_errors, G, _guarded, _hydro_wrench, _k, _ke, NAN, _push, raw,
                              _report, RHO, S_A, S_C, S_IN, S_OUT, S_PV, S_PVO, _same, _same_values, SIZES, step, step_wrench_terms, STEPS, _tiled, _unguard,
                              _untouched)

pytestmark = pytest.mark.gpu


def test_population_covers_the_law(pop):
    st, _, _, _, ctl, _ = pop
    for n in SIZES:
        w = phr.error_quaternion(st[:n], ctl[:n])[:, 3]
        assert (np.abs(w) >= 0.1).all(), (n, np.abs(w).min())    # away from the sign flip, the law's one discontinuity
    w = phr.error_quaternion(st, ctl)[:, 3]
    assert 0.3 < (w < 0).mean() < 0.7
    sat_f, sat_t = phr.saturated(st, ctl)
    assert 0.25 <= (sat_f | sat_t).mean() <= 0.45 and sat_f.mean() > 0.1 and sat_t.mean() > 0.1
    assert np.isfinite(phr.wrench(st, ctl)).all()


# ---- 1. dispatch ---------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_no_control_is_the_applied_entry_and_zero_gains_change_nothing(coeff, implicit, pop, native_built):
    """control = NULL: the bits of hydro_step_fused_tiled_multi_app, with and without `applied`, with and without a log.
    All-zero gains (targets and limits as drawn): its state, prev_out and kinetic-energy pair by value."""
    st, pv, params, applied, ctl, _ = pop
    zero_gains = ctl.copy()
    zero_gains[:, 7:15] = 0.0
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        watched = sorted({b for b in (0, 63, 64, n - 1) if b < n})
        eng.set_watch(watched)
        a, z = _tiled(applied[:n]), _tiled(zero_gains[:n])
        for steps in STEPS:
            for app in (None, a):
                for with_log in (False, True):
                    def logs():
                        return dict(log=torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)) if with_log else {}
                    cur, old = _buffers(st, pv, n)
                    ke0, kw0 = _ke(), logs()
                    eng.step_fused_tiled_multi_applied(cur, old, n, DT, steps, app, "world", implicit_drag=implicit, ke_out=ke0, **kw0)
                    want, want_prev = old, cur[:, 7:13]
                    for control in (None, z):
                        c, o = _buffers(st, pv, n)
                        ke, kw = _ke(), logs()
                        got, got_prev = step(eng, "ctl", c, o, n, steps, control=control, applied=app, implicit=implicit, ke=ke, **kw)
                        torch.cuda.synchronize()
                        what = (n, steps, app is None, with_log, control is None)
                        assert _same_values(got, want) and _same_values(got_prev, want_prev) and _same_values(ke, ke0), what
                        if with_log:
                            assert _same_values(kw["log"], kw0["log"]), what
                        if control is None:
                            assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got_prev), _bits(want_prev)) \
                                and torch.equal(_bits(ke), _bits(ke0)), what
                            assert not with_log or torch.equal(_bits(kw["log"]), _bits(kw0["log"])), what
        # and the plain entry, for zero gains without an applied wrench
        cur, old = _buffers(st, pv, n)
        want = eng.step_fused_tiled_multi(cur, old, n, DT, 2, implicit_drag=implicit)
        c, o = _buffers(st, pv, n)
        got, _ = step(eng, "ctl", c, o, n, 2, control=z, implicit=implicit)
        torch.cuda.synchronize()
        assert _same_values(got, want), n
        eng.close()


# ---- 2. one step against fp64 ------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
@pytest.mark.parametrize("with_applied", [False, True], ids=["hold", "hold+applied"])
def test_one_step_against_fp64(coeff, implicit, with_applied, pop, native_built):
    st, pv, params, applied, ctl, comps = pop
    pr = params[coeff]
    a_host = applied if with_applied else np.zeros_like(applied)
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        cur, old = _buffers(st, pv, n)
        hydro = scenes.from_tiled(_hydro_wrench(eng, cur, old, n).cpu().numpy(), n)
        got, _ = step(eng, "ctl", cur, old, n, 1, control=_tiled(ctl[:n]), applied=_tiled(applied[:n]) if with_applied else None, implicit=implicit)
        torch.cuda.synchronize()
        k = _k(comps(coeff), st, pr, coeff, n) if implicit else None
        worst[n] = fp64_step_errors(scenes.from_tiled(got.cpu().numpy(), n), st[:n], hydro, pr[:n], k, applied=a_host[:n], ctl=ctl[:n])
        eng.close()
    _report(f"pose hold{' + applied' if with_applied else ''} {'implicit' if implicit else 'explicit'} {coeff}", worst)


# ---- 3. the feedback acts at every step of a launch ------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_resident_launch_equals_single_steps_and_is_no_zero_order_hold(coeff, implicit, pop, native_built):
    st, pv, params, applied, ctl, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        a, c17 = _tiled(applied[:n]), _tiled(ctl[:n])
        before = c17.clone()
        cur, old = _buffers(st, pv, n)
        ke7 = _ke()
        got, got_prev = step(eng, "ctl", cur, old, n, 7, control=c17, applied=a, frame="body", implicit=implicit, ke=ke7)
        c, o = _buffers(st, pv, n)
        ke1 = _ke()
        for k in range(7):
            step(eng, "ctl", c, o, n, 1, control=c17, applied=a, frame="body", implicit=implicit, ke=ke1 if k == 6 else None)
            c, o = o, c
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(c)) and torch.equal(_bits(got_prev), _bits(o[:, 7:13])), n
        assert torch.equal(_bits(ke7), _bits(ke1)) and torch.equal(_bits(c17), _bits(before))
        # what a zero-order hold gives: seven steps of the applied entry holding the wrench the law gives at the first state
        held = _tiled(phr.wrench(st[:n], ctl[:n]).astype(np.float32))
        cz, oz = _buffers(st, pv, n)
        eng.step_fused_tiled_multi_applied(cz, oz, n, DT, 7, held, "world", implicit_drag=implicit)
        cf, of = _buffers(st, pv, n)
        fed, _ = step(eng, "ctl", cf, of, n, 7, control=c17, implicit=implicit)
        torch.cuda.synchronize()
        fed, zoh = scenes.from_tiled(fed.cpu().numpy(), n), scenes.from_tiled(oz.cpu().numpy(), n)
        both = np.isfinite(fed).all(axis=1) & np.isfinite(zoh).all(axis=1)   # (seven explicit steps carry some light bodies out of range, body 0 among them)
        assert both.any() or n == 1, n
        assert not both.any() or (fed[both] != zoh[both]).any(axis=1).mean() > 0.9, n
        eng.close()


# ---- 4. directions, by hand ------------------------------------------------------------------------------------------------------------
def test_literal_directions_on_dry_bodies(native_built):
    """Dry bodies (z = +100: the hydrodynamic wrench is exact zeros), mass 2, at rest, dt 0.01: only gravity and the law act.
    Body 0 stands 0.5 m in +x of its target: acceleration -kp e / m along x.  Body 1 is yawed by +30 degrees against its
    target: a torque about -z of kp_ang 2 sin(15 deg).  Body 2 is yawed by -30 degrees: +z.  Body 3 is far from its target
    along (1, 2, 2) / 3 with f_max = 3: acceleration f_max / m along -(1, 2, 2) / 3."""
    from silver2_isaacsim_amd.engine import HydroEngine
    dt, m, kp, kpa, fmax = 0.01, 2.0, 8.0, 0.4, 3.0
    dims = (0.4, 0.3, 0.2)
    iz = m / 12.0 * (dims[0] ** 2 + dims[1] ** 2)
    half = np.radians(15.0)
    st = np.zeros((4, 13), np.float32)
    st[:, 2], st[:, 6] = 100.0, 1.0
    st[0, 0] = 0.5
    st[1, 3:7] = (0.0, 0.0, np.sin(half), np.cos(half))
    st[2, 3:7] = (0.0, 0.0, -np.sin(half), np.cos(half))
    st[3, 0:3] += np.array([1.0, 2.0, 2.0]) * 30.0
    ctl = phr.record(4, (0, 0, 100), (0, 0, 0, 1), kp_lin=np.array([[kp], [0], [0], [kp]]), kp_ang=[0, kpa, kpa, 0],
                     f_max=[np.inf, np.inf, np.inf, fmax])
    pr = np.tile(np.array([[*dims, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, m]], np.float32), (4, 1))
    eng = HydroEngine(4, DEV, RHO, G)
    eng.set_params(pr)
    cur, old = _tiled(st), _tiled(np.zeros((4, 13), np.float32))
    assert (scenes.from_tiled(eng.step_wrench_tiled(cur, 4, dt, prev=old).cpu().numpy(), 4) == 0.0).all()
    eng.step_fused_tiled_multi_controlled(cur, old, 4, dt, 1, _tiled(ctl))
    torch.cuda.synchronize()
    got = scenes.from_tiled(old.cpu().numpy(), 4).astype(np.float64)

    def close(x, want, scale):
        """|x - want| <= 1e-6 of `scale`, per component (8 x 2^-24 is 4.8e-7: a handful of fp32 roundings)."""
        return np.all(np.abs(x - np.asarray(want)) <= 1e-6 * np.asarray(scale))

    fall = -G * dt
    dv = dt * kp * 0.5 / m
    assert close(got[0, 7:10], (-dv, 0.0, fall), (dv, dv, -fall)), got[0, 7:10]
    assert (got[0, 10:13] == 0.0).all()
    dw = dt * kpa * 2.0 * np.sin(half) / iz
    assert close(got[1, 10:13], (0.0, 0.0, -dw), dw) and got[1, 12] < 0, got[1, 10:13]
    assert close(got[2, 10:13], (0.0, 0.0, +dw), dw) and got[2, 12] > 0, got[2, 10:13]
    assert close(got[1, 7:10], (0.0, 0.0, fall), -fall) and close(got[2, 7:10], (0.0, 0.0, fall), -fall)
    da = dt * fmax / m
    assert close(got[3, 7:10], (-da / 3, -2 * da / 3, -2 * da / 3 + fall), (da, da, da - fall)), got[3, 7:10]
    eng.close()


# ---- 5. with the recorder ----------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_recorded_rows_with_a_pose_hold(coeff, implicit, pop, native_built):
    """fields = 19, every = 2, launches of 3 + 3 + 1 steps; watched: bodies 0, 63, 64 and n - 1.  State rows: single stepping
    with the hold, bit for bit.  Wrench rows: step_wrench_tiled(state before) + applied + the fp64 law, each component within
    the bound of the one-step test in units of 2^-24 of its surrogate scale."""
    st, pv, params, applied, ctl, _ = pop
    every, chunk, steps = 2, 3, 7
    worst = 0.0
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        a, c17 = _tiled(applied[:n]), _tiled(ctl[:n])
        watched = sorted({b for b in (0, 63, 64, n - 1) if b < n})
        eng.set_watch(watched)
        c, o = _buffers(st, pv, n)
        states, totals, scales = [], [], []
        for _ in range(steps):
            before = scenes.from_tiled(c.cpu().numpy(), n)
            hydro = scenes.from_tiled(_hydro_wrench(eng, c, o, n).cpu().numpy(), n)
            total, surrogate = step_wrench_terms(before[watched], hydro[watched], applied=applied[:n][watched], ctl=ctl[:n][watched])
            surrogate[:, 3:6] = surrogate[:, 3:4]
            totals.append(total)
            scales.append(surrogate)
            step(eng, "ctl", c, o, n, 1, control=c17, applied=a, implicit=implicit)
            c, o = o, c
            states.append(scenes.from_tiled(c.cpu().numpy(), n)[watched])
        log = torch.full((5, 19, len(watched) + 2), NAN, dtype=torch.float32, device=DEV)
        cur, old = _buffers(st, pv, n)
        done = rows = 0
        while done < steps:
            k = min(chunk, steps - done)
            phase, row0, _ = recorder_cadence(done, every, k)
            rows += eng.step_fused_tiled_multi_controlled(cur, old, n, DT, k, c17, a, "world", log=log, every=every, phase=phase, row0=row0,
                                                          implicit_drag=implicit)
            cur, old = old, cur
            done += k
        torch.cuda.synchronize()
        assert rows == 3
        host = log.cpu().numpy()
        for r, after in enumerate((2, 4, 6)):
            assert np.array_equal(host[r, :13, :len(watched)].T.view(np.uint32), states[after - 1].view(np.uint32)), (n, after)
            gw, ww, sc = host[r, 13:, :len(watched)].T.astype(np.float64), totals[after - 1], scales[after - 1]
            fine = np.isfinite(ww) & np.isfinite(sc)             # (the explicit form may have carried a light body out of range)
            assert (np.isfinite(gw) == np.isfinite(ww))[fine].all(), (n, after)
            err = np.abs(gw - ww)[fine & np.isfinite(gw)] / (io.ULP * sc[fine & np.isfinite(gw)])
            worst = max(worst, float(err.max(initial=0.0)))
        assert np.isnan(host[3:]).all() and np.isnan(host[:, :, len(watched):]).all()
        assert torch.equal(_bits(cur), _bits(c))
        eng.close()
    print(f"[pose hold, recorded wrench {'implicit' if implicit else 'explicit'} {coeff}] max {worst:.2f} ulps of the surrogate scale (bound {B:g})")
    assert worst <= B


# ---- 6. guards and refusals through the raw C ABI ----------------------------------------------------------------------------------


@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """Tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n of every
    buffer, `control` and `applied` included: finite outputs within the bound, no sentinel overwritten, inputs untouched."""
    st, pv, params, applied, ctl, comps = pop
    pr = params[coeff]
    worst = {}
    for n in (65, 4097):
        eng = _engine(n, pr, coeff)
        tiles = (n + 63) // 64
        state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
        before = [b.cpu().numpy() for b in (state, prev, a, c17)]
        out = torch.full((tiles * S_OUT,), NAN, device=DEV)
        pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
        wbuf = _guarded(np.zeros((n, 6), np.float32), 6 * 64 + 8)
        eng._check(eng._lib.hydro_step_wrench_tiled(eng._h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT,
                                                    wbuf.data_ptr(), 6 * 64 + 8, eng._stream(None)))
        rc, written = raw(eng, "ctl", n, state, prev, out, pvo, implicit=implicit, applied=a.data_ptr(), control=c17.data_ptr())
        eng._check(rc)
        torch.cuda.synchronize()
        assert written == 0
        got, rest = _unguard(out, n, 13, S_OUT)
        pv_out, prest = _unguard(pvo, n, 6, S_PVO)
        assert np.isnan(rest).all() and np.isnan(prest).all(), (n, "a sentinel of an output was overwritten")
        assert np.array_equal(pv_out, st[:n, 7:13])
        assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17), before))
        assert np.isfinite(got).all(), (n, "a sentinel was read")
        hydro, _ = _unguard(wbuf, n, 6, 6 * 64 + 8)
        k = _k(comps(coeff), st, pr, coeff, n) if implicit else None
        worst[n] = fp64_step_errors(got, st[:n], hydro, pr[:n], k, applied=applied[:n], ctl=ctl[:n])
        eng.close()
    _report(f"C ABI pose hold {'implicit' if implicit else 'explicit'} {coeff}, strides {S_IN}/{S_OUT}/{S_A}/{S_C}", worst)


def test_refusals_launch_nothing(pop, native_built):
    st, pv, params, applied, ctl, _ = pop
    n = 257
    eng = _engine(n, params["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A), _guarded(ctl[:n], S_C)
    out = torch.full((tiles * max(S_OUT, S_C),), NAN, device=DEV)
    pvo = torch.full((tiles * max(S_PVO, S_C),), NAN, device=DEV)
    log = torch.full((4 * 13 * 8 + tiles * S_C,), NAN, device=DEV)            # (4, 13, 8) rows, and room for a record that starts in it
    E_ARG, E_STATE = -1, -5
    ap, cp = a.data_ptr(), c17.data_ptr()
    for app in (None, ap):
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=cp + 4) == (E_ARG, -7)                # misaligned
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=cp, s_control=1087) == (E_ARG, -7)
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=cp, s_control=1090) == (E_ARG, -7)     # not a multiple of 4
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=cp, s_control=1 << 24) == (E_ARG, -7)
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=out.data_ptr()) == (E_ARG, -7)        # control aliases state_out
        assert raw(eng, "ctl", n, state, prev, out, pvo, applied=app, control=pvo.data_ptr()) == (E_ARG, -7)        # ... prev_out
        assert raw(eng, "ctl", n, state, prev, out, pvo, steps=0, applied=app, control=cp) == (E_ARG, -7)
    assert raw(eng, "ctl", n, state, prev, out, pvo, applied=ap + 4, control=cp) == (E_ARG, -7)                     # what the applied entry refuses
    assert raw(eng, "ctl", n, state, prev, out, pvo, applied=ap, s_applied=383, control=cp) == (E_ARG, -7)
    assert raw(eng, "ctl", n, state, prev, out, pvo, log=log, control=cp) == (E_STATE, -7)            # a log without a watch list
    eng.set_watch([0, 256])
    assert raw(eng, "ctl", n, state, prev, out, pvo, log=log, control=log.data_ptr() + 4 * 13 * 8 * 4 - 64) == (E_ARG, -7)    # control reaches into the log
    assert raw(eng, "ctl", n, state, prev, out, pvo, steps=5, log=log, control=cp) == (E_ARG, -7)     # rows 0 .. 4 of 4
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all()
    # and the legal launches next to them: a record just behind the log; with the log, rows are counted and written
    log[4 * 13 * 8:] = c17
    assert raw(eng, "ctl", n, state, prev, out, pvo, steps=3, log=log, control=log.data_ptr() + 4 * 13 * 8 * 4) == (0, 3)
    torch.cuda.synchronize()
    state3, _ = _unguard(out[:tiles * S_OUT], n, 13, S_OUT)
    rows = log[:4 * 13 * 8].view(4, 13, 8)
    assert not np.isnan(state3).all() and torch.isnan(rows[3:]).all() and torch.isnan(rows[:, :, 2:]).all()
    assert np.array_equal(rows[2, :, :2].cpu().numpy().T, state3[[0, 256]], equal_nan=True)   # the last row is the final state
    eng.close()


# ---- 7. ClosedLoopSim ------------------------------------------------------------------------------------------------------------
def _c2():
    return scenes.scene_c2(n=257)


def _hold(sc, seed):
    """set_pose_hold arguments for every body of `sc`: targets near the start, gains per unit mass, some limits that bind."""
    rng = np.random.default_rng(seed)
    m = sc.params[:, 10:11].astype(np.float64)
    inertia = io.box_inertia(sc.params.astype(np.float64)).mean(axis=1)
    q = sc.state[:, 3:7].astype(np.float64) + rng.normal(0.0, 0.2, (sc.n, 4))
    return dict(position=sc.state[:, 0:3] + rng.uniform(-1.0, 1.0, (sc.n, 3)), orientation_xyzw=q / np.linalg.norm(q, axis=1, keepdims=True),
                kp_lin=m * rng.uniform(5.0, 30.0, (sc.n, 3)), kd_lin=m * 6.0, kp_ang=inertia * 20.0, kd_ang=inertia * 5.0,
                f_max=np.where(np.arange(sc.n) % 3 == 0, 2.0 * m[:, 0], np.inf), t_max=np.inf)


def test_sim_runners_agree_with_a_pose_hold(native_built):
    sc = _c2()
    hold = _hold(sc, 1)
    finals = {}
    for name, go in (("resident", lambda s: s.run_resident(128, chunk=64)), ("eager", lambda s: s.run_eager(128)),
                     ("graph", lambda s: s.run(128, graph_steps=4))):
        sim = ClosedLoopSim(sc)
        buf = sim.set_pose_hold(**hold)
        assert buf is sim.control and tuple(buf.shape) == (5, 17, 64)
        rec = scenes.from_tiled(buf.cpu().numpy(), sc.n)
        assert np.array_equal(rec[:, 0:3], hold["position"].astype(np.float32)) and np.array_equal(rec[:, 15], hold["f_max"].astype(np.float32))
        assert np.array_equal(rec[:, 13], hold["kp_ang"].astype(np.float32)) and np.isinf(rec[:, 16]).all()
        go(sim)
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc)
    plain.run_resident(128, chunk=64)
    assert _same(finals["resident"], finals["eager"]) and _same(finals["resident"], finals["graph"])
    assert np.isfinite(finals["resident"]).all() and not np.array_equal(finals["resident"], plain.state())
    plain.close()


def test_sim_with_applied_wrench_recorder_and_monitor(native_built):
    """A pose hold, an applied wrench, a recorder and a kinetic-energy monitor together: run_resident(chunk=64), run_eager
    and - without the recorder, which cannot ride in a graph - graph replays give the same bits and the same samples."""
    sc = _c2()
    hold, w = _hold(sc, 2), _push(sc, 2)
    a, b, g = (ClosedLoopSim(sc, ke_every=64) for _ in range(3))
    for s in (a, b, g):
        s.set_pose_hold(**hold)
        s.set_applied_wrench(w)
    rec = a.record([256, 0, 64], every=32, rows=8, wrench=True)
    a.run_resident(128, chunk=64)
    rows = []
    for k in range(128):
        b.run_eager(1)
        if (k + 1) % 32 == 0:
            rows.append(b.state()[[256, 0, 64]])
    g.run(128, graph_steps=64)
    assert _same(a.state(), b.state()) and _same(a.state(), g.state()) and _same(rec.states(), np.stack(rows))
    for s in (a, b, g):
        s.monitor.collect(block=True)
    assert len(a.monitor.samples) == 2 and a.monitor.samples == b.monitor.samples == g.monitor.samples
    for s in (a, b, g):
        s.close()


def test_rewriting_the_record_between_graph_replays(native_built):
    sc = _c2()
    h1, h2 = _hold(sc, 3), _hold(sc, 4)
    g, e, held = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    for s in (g, e, held):
        s.set_pose_hold(**h1)
    g.run(4, graph_steps=4)
    address, graph = g.control.data_ptr(), g._graph
    e.run_eager(4)
    e.set_pose_hold(**h2)
    with torch.cuda.stream(g.stream):                            # the next set-points, written on the device
        g.control.copy_(e.control)
    g.run(4, graph_steps=4)
    assert g._graph is graph and g.control.data_ptr() == address  # a replay of the same graph, reading the same buffer
    e.run_eager(4)
    held.run(8, graph_steps=4)
    assert _same(g.state(), e.state()) and not np.array_equal(g.state(), held.state())
    for s in (g, e, held):
        s.close()


def test_partial_hold_clear_and_refusals(native_built):
    sc = _c2()
    hold = _hold(sc, 5)
    some, none, cleared = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    m = sc.params[[3, 200], 10:11].astype(np.float64)
    buf = some.set_pose_hold(position=sc.state[[3, 200], 0:3] + 0.5, kp_lin=m * 20.0, kd_lin=m * 4.0, bodies=[3, 200])
    rec = scenes.from_tiled(buf.cpu().numpy(), sc.n)
    others = np.setdiff1d(np.arange(sc.n), [3, 200])
    assert (rec[others, 7:15] == 0.0).all() and np.array_equal(rec[[3, 200], 3:7], sc.state[[3, 200], 3:7])   # default: the current attitude
    some.run_resident(12, chunk=4)
    none.run_resident(12, chunk=4)
    got, want = some.state(), none.state()
    assert _same_values(torch.from_numpy(got[others]), torch.from_numpy(want[others])) and not np.array_equal(got[[3, 200]], want[[3, 200]])
    cleared.set_pose_hold(**hold)
    assert cleared.control is not None
    cleared.clear_pose_hold()
    assert cleared.control is None and cleared._graph is None
    cleared.run_resident(8, chunk=4)
    cleared.run(4, graph_steps=4)
    assert _same(cleared.state(), want)
    for s in (some, none, cleared):
        s.close()
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_pose_hold(kp_lin=1.0)
    two_kernel.close()
    sim = ClosedLoopSim(sc)
    for bad in (dict(position=sc.state[:5, 0:3]), dict(kp_lin=np.ones((sc.n, 2))), dict(kp_lin=1.0, bodies=[1, 257]),
                dict(kp_ang=np.ones(3), bodies=[1, 2]), dict(f_max=-1.0), dict(kp_lin=float("nan"))):
        with pytest.raises(ValueError):
            sim.set_pose_hold(**bad)
    assert sim.control is None
    sim.close()


# ---- 8. the example ----------------------------------------------------------------------------------------------------------------
def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rov_station_keeping_example(native_built):
    """The law in the kernel at chunk = 60 against no controller, and against the same law between launches at chunk = 4
    (examples/rov_depth_hold.py): applied four times as often it must not lose."""
    keep, between = _example("rov_station_keeping"), _example("rov_depth_hold")
    on = keep.main(steps=240, bodies=256, chunk=60)
    off = keep.main(steps=240, bodies=256, chunk=60, control=False)
    outer = between.main(steps=240, bodies=256, chunk=4)
    assert on["state"].shape == (256, 13) and np.isfinite(on["state"]).all() and np.isfinite(off["state"]).all()
    assert np.array_equal(on["setpoint"], outer["setpoint"])
    print(f"[rov_station_keeping] mean depth error {on['start_error']:.3f} m -> {on['depth_error']:.5f} m with the pose hold at chunk 60, "
          f"{off['depth_error']:.4f} m without, {outer['depth_error']:.5f} m with the between-launch controller at chunk 4")
    assert on["depth_error"] < off["depth_error"]
    assert on["depth_error"] <= outer["depth_error"]
