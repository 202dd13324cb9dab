"""The applied wrench on the device (hydro_step_fused_tiled_multi_app): a zero wrench changes nothing; in the world frame
the step is, bit for bit, wrench kernel -> fp32 add -> integrator kernel; both frames follow the fp64 step within the
project's own bound; the direction of a body-frame force and torque is checked against literal expectations (R, not R^T);
a resident launch equals single stepping; the recorder logs the total wrench; guards, refusals, ClosedLoopSim, the example.

Bound of the fp64 comparisons: integrator_oracle.STEP_ULP_BOUND (24), with the scales of field_scales on a surrogate wrench
|F_hydro,i| + |f_applied|, |tau_hydro| + |tau_applied| - a thrust that cancels the water does not shrink the yardstick.
Each of those tests prints its largest error per group."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import populations
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.engine import HydroEngine
from silver2_isaacsim_amd.simulate import ClosedLoopSim, recorder_cadence
from resident_harness import (_bits, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, FRAMES, G, _guarded, _hydro_wrench, _k, _ke,
                              NAN, _push, raw, _report, RHO, S_A, S_IN, S_OUT, S_PV, S_PVO, _same, _same_values, SIZES, step, STEPS, _tiled, _unguard,
                              _untouched)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pop():
    """The designed population at the largest size, its parameters per coefficient format, an applied wrench of the size of
    the hydrodynamic one (forces up to 50 N per kg of body mass per component, torques up to that times the largest edge)
    and, per coefficient format, the components of the oracle that drag_jacobian needs."""
    st, pv, pr = populations.integrator_population(n=max(SIZES), seed=31)
    params = {"f32": pr, "f16": pr.copy()}
    params["f16"][:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(77)
    top = 50.0 * pr[:, 10:11].astype(np.float64)
    applied = np.concatenate([rng.uniform(-1, 1, (len(st), 3)) * top,
                              rng.uniform(-1, 1, (len(st), 3)) * top * pr[:, 0:3].max(axis=1, keepdims=True)], axis=1).astype(np.float32)
    cache = {}

    def comps(coeff):
        if coeff not in cache:
            cache[coeff] = ho.step_wrench(st, pv, params[coeff], RHO, G, DT)[2]
        return cache[coeff]
    return st, pv, params, applied, comps


# ---- 1. zero is nothing ------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_zero_wrench_is_the_plain_step(coeff, implicit, pop, native_built):
    """applied = 0 in either frame: state, prev_out and the kinetic-energy pair of hydro_step_fused_tiled_multi, by value
    (x + 0 == x; the sign of a zero is not a difference).  applied = NULL: the same bits."""
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        zero = eng.alloc_tiled(6, n)
        for steps in STEPS:
            cur, old = _buffers(st, pv, n)
            ke0 = _ke()
            want = eng.step_fused_tiled_multi(cur, old, n, DT, steps, implicit_drag=implicit, ke_out=ke0)
            want_prev = cur[:, 7:13]
            for applied, frame in ((zero, "world"), (zero, "body"), (None, "world"), (None, "body")):
                c, o = _buffers(st, pv, n)
                ke = _ke()
                got, got_prev = step(eng, "app", c, o, n, steps, applied=applied, frame=frame, implicit=implicit, ke=ke)
                torch.cuda.synchronize()
                assert _same_values(got, want) and _same_values(got_prev, want_prev) and _same_values(ke, ke0), (n, steps, frame, applied is None)
                if applied is None:
                    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got_prev), _bits(want_prev)) \
                        and torch.equal(_bits(ke), _bits(ke0))
            if steps == 1:
                assert not torch.isnan(ke0).any() and not torch.isnan(want).any()
        eng.close()


# ---- 2. world frame = wrench kernel, fp32 add, integrator kernel ---------------------------------------------------------------
@COEFFS_SEMANTICS
def test_world_frame_is_the_two_kernel_path_bit_for_bit(coeff, semantics, pop, native_built):
    st, pv, params, applied, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        a = _tiled(applied[:n])
        cur, old = _buffers(st, pv, n)
        total = _hydro_wrench(eng, cur, old, n) + a                 # torch: one fp32 add per component
        want = eng.integrate_tiled(cur, total, n, DT)
        got, _ = step(eng, "app", cur, old, n, 1, applied=a)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)), n
        assert (total != _hydro_wrench(eng, cur, old, n)).any()
        eng.close()


# ---- 3. against fp64 ----------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
@pytest.mark.parametrize("frame", FRAMES)
def test_one_step_against_fp64(coeff, implicit, frame, pop, native_built):
    st, pv, params, applied, comps = pop
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        cur, old = _buffers(st, pv, n)
        hydro = scenes.from_tiled(_hydro_wrench(eng, cur, old, n).cpu().numpy(), n)
        got, _ = step(eng, "app", cur, old, n, 1, applied=_tiled(applied[:n]), frame=frame, implicit=implicit)
        torch.cuda.synchronize()
        k = _k(comps(coeff), st, pr, coeff, n) if implicit else None
        worst[n] = fp64_step_errors(scenes.from_tiled(got.cpu().numpy(), n), st[:n], hydro, pr[:n], k, applied=applied[:n], frame=frame)
        eng.close()
    _report(f"applied {frame} {'implicit' if implicit else 'explicit'} {coeff}", worst)


# ---- 4. direction, by hand ----------------------------------------------------------------------------------------------------
def test_direction_of_a_body_frame_force_and_torque(native_built):
    """One dry body (z = +100: its hydrodynamic wrench is exact zeros), mass 2, at rest, turned 90 degrees about z, dt 0.01.
    A body-frame force along body x accelerates it along WORLD y, the same numbers in the world frame along world x; a
    body-frame torque about body x spins it about world y.  Literal expectations: R versus R^T."""
    dt, m, F, tau = 0.01, 2.0, 3.0, 0.5
    dims = (0.4, 0.3, 0.2)
    ix, iy = m / 12.0 * (dims[1] ** 2 + dims[2] ** 2), m / 12.0 * (dims[0] ** 2 + dims[2] ** 2)
    st = np.zeros((1, 13), np.float32)
    st[0, 2] = 100.0
    st[0, 3:7] = (0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5))
    pr = np.array([[*dims, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, m]], np.float32)
    eng = HydroEngine(1, DEV, RHO, G)
    eng.set_params(pr)
    cur, old = _tiled(st), _tiled(np.zeros((1, 13), np.float32))
    assert (scenes.from_tiled(eng.step_wrench_tiled(cur, 1, dt, prev=old).cpu().numpy(), 1) == 0.0).all()

    def step(a, frame):
        c, o = cur.clone(), old.clone()
        eng.step_fused_tiled_multi_applied(c, o, 1, dt, 1, _tiled(np.array([a], np.float32)), frame)
        torch.cuda.synchronize()
        return scenes.from_tiled(o.cpu().numpy(), 1)[0].astype(np.float64)

    def close(got, want, scale):
        """|got - want| <= 1e-6 of `scale`, per component (8 x 2^-24 is 4.8e-7: a handful of fp32 roundings)."""
        return np.all(np.abs(got - np.asarray(want)) <= 1e-6 * np.asarray(scale))

    dv, fall = dt * F / m, -G * dt
    body, world = step((F, 0, 0, 0, 0, 0), "body"), step((F, 0, 0, 0, 0, 0), "world")
    assert close(body[7:10], (0.0, dv, fall), (dv, dv, -fall)), body[7:10]
    assert close(world[7:10], (dv, 0.0, fall), (dv, dv, -fall)), world[7:10]
    assert (body[10:13] == 0.0).all() and (world[10:13] == 0.0).all()
    body, world = step((0, 0, 0, tau, 0, 0), "body"), step((0, 0, 0, tau, 0, 0), "world")
    assert close(body[10:13], (0.0, dt * tau / ix, 0.0), dt * tau / ix), body[10:13]    # body x is world y; about body x the inertia is ix
    assert close(world[10:13], (dt * tau / iy, 0.0, 0.0), dt * tau / iy), world[10:13]  # world x is body -y; about body y it is iy
    assert close(body[7:10], (0.0, 0.0, fall), -fall) and close(world[7:10], (0.0, 0.0, fall), -fall)
    eng.close()


# ---- 5. resident = single stepping ----------------------------------------------------------------------------------------------
@COEFFS
@DRAG
@pytest.mark.parametrize("frame", FRAMES)
def test_resident_launch_equals_single_steps(coeff, implicit, frame, pop, native_built):
    st, pv, params, applied, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        a = _tiled(applied[:n])
        before = a.clone()
        cur, old = _buffers(st, pv, n)
        ke7 = _ke()
        got, got_prev = step(eng, "app", cur, old, n, 7, applied=a, frame=frame, implicit=implicit, ke=ke7)
        c, o = _buffers(st, pv, n)
        ke1 = _ke()
        for k in range(7):
            step(eng, "app", c, o, n, 1, applied=a, frame=frame, implicit=implicit, ke=ke1 if k == 6 else None)
            c, o = o, c
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(c)) and torch.equal(_bits(got_prev), _bits(o[:, 7:13])), (n, frame)
        assert _same_values(ke7, ke1)
        assert torch.equal(_bits(a), _bits(before))
        eng.close()


# ---- 6. with the recorder ----------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_recorded_rows_with_an_applied_wrench(coeff, implicit, pop, native_built):
    """fields = 19, every = 2, launches of 3 + 3 + 1 steps; watched: bodies 0, 63, 64 and n - 1.  State rows: single stepping
    with the applied wrench, bit for bit, in both frames.  Wrench rows in the world frame: step_wrench_tiled(state before) + a."""
    st, pv, params, applied, _ = pop
    every, chunk, steps = 2, 3, 7
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff)
        a = _tiled(applied[:n])
        watched = sorted({b for b in (0, 63, 64, n - 1) if b < n})
        eng.set_watch(watched)
        for frame in FRAMES:
            # single stepping: the state after every step, and the total wrench of every step
            c, o = _buffers(st, pv, n)
            states, wrenches = [], []
            for _ in range(steps):
                wrenches.append(scenes.from_tiled((_hydro_wrench(eng, c, o, n) + a).cpu().numpy(), n)[watched])
                step(eng, "app", c, o, n, 1, applied=a, frame=frame, implicit=implicit)
                c, o = o, c
                states.append(scenes.from_tiled(c.cpu().numpy(), n)[watched])
            log = torch.full((5, 19, len(watched) + 2), NAN, dtype=torch.float32, device=DEV)
            cur, old = _buffers(st, pv, n)
            done = rows = 0
            while done < steps:
                k = min(chunk, steps - done)
                phase, row0, _ = recorder_cadence(done, every, k)
                rows += eng.step_fused_tiled_multi_applied(cur, old, n, DT, k, a, frame, log=log, every=every, phase=phase, row0=row0,
                                                           implicit_drag=implicit)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            assert rows == 3
            host = log.cpu().numpy()
            for r, after in enumerate((2, 4, 6)):
                assert np.array_equal(host[r, :13, :len(watched)].T.view(np.uint32), states[after - 1].view(np.uint32)), (n, frame, after)
                if frame == "world":
                    gw, ww = host[r, 13:, :len(watched)].T, wrenches[after - 1]
                    assert ((gw.view(np.uint32) == ww.view(np.uint32)) | (np.isnan(gw) & np.isnan(ww))).all(), (n, after)
            assert np.isnan(host[3:]).all() and np.isnan(host[:, :, len(watched):]).all()
            assert torch.equal(_bits(cur), _bits(c))
        eng.close()


# ---- 7. guards and refusals through the raw C ABI ----------------------------------------------------------------------------------


@COEFFS
@DRAG
@pytest.mark.parametrize("frame", FRAMES)
def test_strides_and_nan_guards(coeff, implicit, frame, pop, native_built):
    """Tile strides larger than F * 64 and different for every buffer, NaN in the stride padding and past body n of every
    buffer, `applied` included: finite outputs within the bound, no sentinel overwritten, inputs untouched."""
    st, pv, params, applied, comps = pop
    pr = params[coeff]
    worst = {}
    for n in (65, 4097):
        eng = _engine(n, pr, coeff)
        tiles = (n + 63) // 64
        state, prev, a = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A)
        before = [b.cpu().numpy() for b in (state, prev, a)]
        out = torch.full((tiles * S_OUT,), NAN, device=DEV)
        pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
        wbuf = _guarded(np.zeros((n, 6), np.float32), 6 * 64 + 8)
        eng._check(eng._lib.hydro_step_wrench_tiled(eng._h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT,
                                                    wbuf.data_ptr(), 6 * 64 + 8, eng._stream(None)))
        rc, written = raw(eng, "app", n, state, prev, out, pvo, implicit=implicit, frame=FRAMES.index(frame), applied=a.data_ptr())
        eng._check(rc)
        torch.cuda.synchronize()
        assert written == 0
        got, rest = _unguard(out, n, 13, S_OUT)
        pv_out, prest = _unguard(pvo, n, 6, S_PVO)
        assert np.isnan(rest).all() and np.isnan(prest).all(), (n, "a sentinel of an output was overwritten")
        assert np.array_equal(pv_out, st[:n, 7:13])
        assert all(_untouched(b, was) for b, was in zip((state, prev, a), before))
        assert np.isfinite(got).all(), (n, "a sentinel was read")
        hydro, _ = _unguard(wbuf, n, 6, 6 * 64 + 8)
        k = _k(comps(coeff), st, pr, coeff, n) if implicit else None
        worst[n] = fp64_step_errors(got, st[:n], hydro, pr[:n], k, applied=applied[:n], frame=frame)
        eng.close()
    _report(f"C ABI applied {frame} {'implicit' if implicit else 'explicit'} {coeff}, strides {S_IN}/{S_OUT}/{S_A}", worst)


def test_refusals_launch_nothing(pop, native_built):
    st, pv, params, applied, _ = pop
    n = 257
    eng = _engine(n, params["f32"], "f32")
    tiles = (n + 63) // 64
    state, prev, a = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(applied[:n], S_A)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    E_ARG, E_STATE = -1, -5
    assert raw(eng, "app", n, state, prev, out, pvo, applied=a.data_ptr() + 4) == (E_ARG, -7)          # misaligned
    assert raw(eng, "app", n, state, prev, out, pvo, applied=a.data_ptr(), s_applied=383) == (E_ARG, -7)
    assert raw(eng, "app", n, state, prev, out, pvo, frame=2, applied=a.data_ptr()) == (E_ARG, -7)
    assert raw(eng, "app", n, state, prev, out, pvo, frame=-1, applied=a.data_ptr()) == (E_ARG, -7)
    assert raw(eng, "app", n, state, prev, out, pvo, applied=out.data_ptr(), s_applied=S_OUT) == (E_ARG, -7)     # applied aliases state_out
    assert raw(eng, "app", n, state, prev, out, pvo, applied=pvo.data_ptr(), s_applied=S_PVO) == (E_ARG, -7)     # ... prev_out
    assert raw(eng, "app", n, state, prev, out, pvo, log=log, applied=a.data_ptr()) == (E_STATE, -7)          # a log without a watch list
    assert raw(eng, "app", n, state, prev, out, pvo, steps=0, applied=a.data_ptr()) == (E_ARG, -7)
    eng.set_watch([0, 256])
    assert raw(eng, "app", n, state, prev, out, pvo, log=log, applied=log.data_ptr()) == (E_ARG, -7)          # applied aliases the log
    assert raw(eng, "app", n, state, prev, out, pvo, steps=5, log=log, applied=a.data_ptr()) == (E_ARG, -7)   # rows 0 .. 4 of 4
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pvo).all() and torch.isnan(log).all()
    # and the legal launch next to them: with the log, rows are counted and written
    assert raw(eng, "app", n, state, prev, out, pvo, steps=3, log=log, applied=a.data_ptr()) == (0, 3)
    torch.cuda.synchronize()
    state3, rest = _unguard(out, n, 13, S_OUT)
    assert not np.isnan(state3).all() and np.isnan(rest).all() and torch.isnan(log[3:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert np.array_equal(log[2, :, :2].cpu().numpy().T, state3[[0, 256]], equal_nan=True)       # the last row is the final state
    eng.close()


# ---- 8. ClosedLoopSim ------------------------------------------------------------------------------------------------------------
def _c2():
    return scenes.scene_c2(n=257)


@pytest.mark.parametrize("frame", FRAMES)
def test_sim_runners_agree_with_a_wrench_set(frame, native_built):
    sc = _c2()
    w = _push(sc, 1)
    finals = {}
    for name, go in (("resident", lambda s: s.run_resident(12, chunk=4)), ("eager", lambda s: s.run_eager(12)),
                     ("graph", lambda s: s.run(12, graph_steps=4))):
        sim = ClosedLoopSim(sc)
        buf = sim.set_applied_wrench(w, frame=frame)
        assert buf is sim.applied and tuple(buf.shape) == (5, 6, 64) and sim.applied_frame == frame
        assert np.array_equal(scenes.from_tiled(buf.cpu().numpy(), sc.n), w)
        go(sim)
        finals[name] = sim.state()
        sim.close()
    plain = ClosedLoopSim(sc)
    plain.run_resident(12, chunk=4)
    assert _same(finals["resident"], finals["eager"]) and _same(finals["resident"], finals["graph"])
    assert not np.array_equal(finals["resident"], plain.state())
    plain.close()


def test_sim_with_recorder_and_monitor(native_built):
    """run_resident with a wrench set, with a recorder and a kinetic-energy monitor attached: the states and samples of eager
    stepping with the same wrench, the recorded rows its states."""
    sc = _c2()
    w = _push(sc, 2)
    a, b = ClosedLoopSim(sc, ke_every=4), ClosedLoopSim(sc, ke_every=4)
    a.set_applied_wrench(torch.from_numpy(w).to(DEV))            # a device tensor
    b.set_applied_wrench(w)
    rec = a.record([256, 0, 64], every=3, rows=8, wrench=True)
    a.run_resident(12, chunk=4)
    rows = []
    for k in range(12):
        b.run_eager(1)
        if (k + 1) % 3 == 0:
            rows.append(b.state()[[256, 0, 64]])
    assert _same(a.state(), b.state()) and _same(rec.states(), np.stack(rows))
    a.monitor.collect(block=True); b.monitor.collect(block=True)
    assert len(a.monitor.samples) == 3 and a.monitor.samples == b.monitor.samples
    a.close(); b.close()


def test_rewriting_the_buffer_between_graph_replays(native_built):
    sc = _c2()
    w1, w2 = _push(sc, 3), _push(sc, 4)
    g, e, held = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    for s in (g, e, held):
        s.set_applied_wrench(w1)
    g.run(4, graph_steps=4)
    address = g.applied.data_ptr()
    with torch.cuda.stream(g.stream):                            # the next command, written on the device
        g.applied.copy_(_tiled(w2))
    graph = g._graph
    g.run(4, graph_steps=4)
    assert g._graph is graph and g.applied.data_ptr() == address  # a replay of the same graph, reading the same buffer
    e.run_eager(4)
    e.set_applied_wrench(w2)
    e.run_eager(4)
    held.run(8, graph_steps=4)
    assert _same(g.state(), e.state()) and not np.array_equal(g.state(), held.state())
    for s in (g, e, held):
        s.close()


def test_partial_wrench_clear_and_refusals(native_built):
    sc = _c2()
    w = _push(sc, 5)
    some, none, cleared = ClosedLoopSim(sc), ClosedLoopSim(sc), ClosedLoopSim(sc)
    some.set_applied_wrench(w[[3, 200]], frame="world", bodies=[3, 200])
    some.run_resident(12, chunk=4)
    none.run_resident(12, chunk=4)
    others = np.setdiff1d(np.arange(sc.n), [3, 200])
    got, want = some.state(), none.state()
    assert _same(got[others], want[others]) and not np.array_equal(got[[3, 200]], want[[3, 200]])
    cleared.set_applied_wrench(w)
    cleared.clear_applied_wrench()
    assert cleared.applied is None
    cleared.run_resident(8, chunk=4)
    cleared.run(4, graph_steps=4)
    assert _same(cleared.state(), want)
    for s in (some, none, cleared):
        s.close()
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.set_applied_wrench(w)
    two_kernel.close()
    sim = ClosedLoopSim(sc)
    for bad in (dict(wrench=w[:5]), dict(wrench=w, frame="local"), dict(wrench=w[:2], bodies=[1, 257]), dict(wrench=w[:3], bodies=[1, 2])):
        with pytest.raises(ValueError):
            sim.set_applied_wrench(**bad)
    assert sim.applied is None
    sim.close()


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------
def test_rov_depth_hold_example(native_built):
    spec = importlib.util.spec_from_file_location("rov_depth_hold", os.path.join(REPO, "examples", "rov_depth_hold.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    on, off = mod.main(steps=240, bodies=256), mod.main(steps=240, bodies=256, control=False)
    assert on["state"].shape == (256, 13) and np.isfinite(on["state"]).all() and np.isfinite(off["state"]).all()
    print(f"[rov_depth_hold] mean depth error {on['start_error']:.3f} m -> {on['depth_error']:.4f} m with the controller, "
          f"{off['depth_error']:.4f} m without")
    assert on["depth_error"] < off["depth_error"]
