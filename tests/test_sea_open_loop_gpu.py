"""The sea in the open-loop entries on the device (hydro_step_wrench_tiled_sea, hydro_step_wrench_aos_sea) and in the plugin:
the time path is hydro_sea_sample's, bit for bit; a step is, bit for bit, the parent entry on the relative state built on the
host from that sample, and the engine's record keeps the TRUE velocity; one explicit closed-loop step is this wrench followed
by the integrator; the fp64 oracle on the relative state within the project's gate; no sea, a still sea and a flat wave are
the parents; refusals launch nothing; a captured launch replays; the plugin applies what a direct call on a second engine
gives at the times 0, dt0, dt0 + dt1; the example.

Population and SEA are those of tests/test_sea_gpu.py.  The view's own error is bounded there (VIEW_BOUND) and reaches these
entries through the sample identity (test 1) - no new number here.  The fp64 gate is the project's 1e-5 of
hydro_oracle.wrench_error: the kernel's arithmetic is the parent's on the inputs the device formed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sea_reference as sr
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import behavior as hb
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.engine import HydroEngine
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.testing import build_main_scene
from designed_populations import hold_pop, SEA, sea_pop as pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import (_buffers, COEFFS_SEMANTICS, DEV, DT, _engine, G, _guarded, NAN, RHO, S_IN, S_PV, _same_bits, SIZES, _tiled, _unguard, _untouched,
                              VIEW_STEPS)

pytestmark = pytest.mark.gpu
assert SIZES == (1, 63, 64, 65, 257, 4097)
GATE = 1e-5                                                       # the project's gate on hydro_oracle.wrench_error
TIMES = tuple(float(step) * DT for step in VIEW_STEPS) + (0.123456789,)     # fp64 products step * DT, and no multiple of DT
S_WR = 6 * 64 + 44                                                # the wrench's tile stride in the guard tests
E_ARG = -1


def _rows(st, n, xyzw):
    """The simulator's tensors of bodies 0 .. n - 1: positions, orientations (wxyz, or xyzw), velocities."""
    q = st[:n, 3:7] if xyzw else st[:n, [6, 3, 4, 5]]
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (st[:n, 0:3], q, st[:n, 7:13]))


def _relative_at(eng, st, pv, n, time):
    """(s_rel, pv_rel) built on the host in fp32 from sea_sample_at's output."""
    w = scenes.from_tiled(eng.sea_sample_at(_tiled(st[:n]), n, time).cpu().numpy(), n)
    return sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])


def _prev_is(eng, v6):
    """The engine-owned previous velocity holds exactly the (n, 6) rows `v6`."""
    return np.array_equal(eng.get_prev_velocity().cpu().numpy().T.view(np.uint32), np.ascontiguousarray(v6).view(np.uint32))


# ---- 1. the time path is the sample's ---------------------------------------------------------------------------------------------
def test_sample_at_time_is_the_sample_at_that_step(pop, native_built):
    st, _, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params["f32"], "f32")
        eng.set_sea(SEA)
        cur = _tiled(st[:n])
        for step in VIEW_STEPS:
            t = float(step) * DT                                  # the fp64 product sea_water forms from (step, DT)
            assert _same_bits(eng.sea_sample_at(cur, n, t), eng.sea_sample(cur, n, step, DT)), (n, step)
        eng.close()


# ---- 2. the step is the parent on the relative state -----------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_step_is_the_parent_entry_on_the_relative_state(coeff, semantics, pop, native_built):
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea(SEA)
        true_state, true_prev, true_vel = _tiled(st[:n]), _tiled(pv[:n]), st[:n, 7:13]
        for time in TIMES:
            s_rel, pv_rel = _relative_at(eng, st, pv, n, time)
            assert (s_rel[:, 2] != st[:n, 2]).mean() > 0.9 or n == 1
            rel_state = _tiled(s_rel)
            # caller-owned previous velocity
            want = eng.step_wrench_tiled(rel_state, n, DT, prev=_tiled(pv_rel))
            assert _same_bits(eng.step_wrench_tiled_sea(true_state, n, DT, time, prev=true_prev), want), (n, time)
            # engine-owned: the same wrench, and the record receives the TRUE velocity
            eng.set_prev_velocity(pv_rel)
            assert _same_bits(eng.step_wrench_tiled(rel_state, n, DT), want)
            eng.set_prev_velocity(pv[:n])
            assert _same_bits(eng.step_wrench_tiled_sea(true_state, n, DT, time), want), (n, time)
            assert _prev_is(eng, true_vel), (n, time)
            # the simulator's rows, in either quaternion order
            want_f, want_t = eng.unpack_wrench_aos(want, n)
            for xyzw in (False, True):
                eng.set_prev_velocity(pv[:n])
                f, t = eng.step_wrench_aos_sea(*_rows(st, n, xyzw), DT, time, quat_xyzw=xyzw)
                assert _same_bits(f, want_f) and _same_bits(t, want_t), (n, time, xyzw)
                assert _prev_is(eng, true_vel), (n, time, xyzw)
            if time == TIMES[1]:                                  # and the parent array-of-structs entry on the relative rows
                eng.set_prev_velocity(pv_rel)
                f, t = eng.step_wrench_aos(*_rows(s_rel, n, False), DT)
                assert _same_bits(f, want_f) and _same_bits(t, want_t), n
        eng.close()


# ---- 3. link to the closed loop --------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_explicit_closed_loop_step_is_this_wrench_then_the_integrator(coeff, semantics, pop, native_built):
    st, pv, params, _, _ = pop
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        eng.set_sea(SEA)
        for step0 in (0, 7, 10 ** 6):
            cur, old = _buffers(st, pv, n)
            wrench = eng.step_wrench_tiled_sea(cur, n, DT, float(step0) * DT, prev=old)
            want = eng.integrate_tiled(cur, wrench, n, DT)
            eng.step_fused_tiled_multi_sea(cur, old, n, DT, 1, step0)
            torch.cuda.synchronize()
            assert _same_bits(old, want), (n, step0)
        eng.close()


# ---- 4. fp64 -----------------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_wrench_against_the_fp64_oracle_on_the_relative_state(coeff, semantics, pop, native_built):
    """hydro_oracle.step_wrench on the fp32 relative state the device formed (test 2: the host-built one, bit for bit), error by
    hydro_oracle.wrench_error, gate 1e-5: the parent kernel's arithmetic on those inputs."""
    st, pv, params, _, _ = pop
    n, time = max(SIZES), 7.0 * DT
    eng = _engine(n, params[coeff], coeff, semantics)
    eng.set_sea(SEA)
    s_rel, pv_rel = _relative_at(eng, st, pv, n, time)
    got = scenes.from_tiled(eng.step_wrench_tiled_sea(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n])).cpu().numpy(), n)
    eng.set_prev_velocity(pv[:n])
    f, t = eng.step_wrench_aos_sea(*_rows(st, n, False), DT, time)
    eng.close()
    ref_f, ref_t, _ = ho.step_wrench(s_rel, pv_rel, params[coeff][:n], RHO, G, DT, semantics=semantics)
    err = ho.wrench_error(got[:, 0:3], got[:, 3:6], ref_f, ref_t, params[coeff][:n], RHO, G)
    err_aos = ho.wrench_error(f.cpu().numpy(), t.cpu().numpy(), ref_f, ref_t, params[coeff][:n], RHO, G)
    print(f"[open-loop sea, {coeff} {semantics}] largest wrench_error against fp64 on the relative state: tiled {err.max():.3e}, rows {err_aos.max():.3e} (gate {GATE:g})")
    assert err.max() <= GATE and err_aos.max() <= GATE, (err.max(), err_aos.max())


# ---- 5. degenerate seas --------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_no_sea_a_still_sea_and_a_flat_wave_are_the_parents(coeff, semantics, pop, native_built):
    st, pv, params, _, _ = pop
    still = SeaState()
    flat = SeaState().add_wave(0.0, 0.3, -0.2, 1.7, 0.4)
    for n in SIZES:
        eng = _engine(n, params[coeff], coeff, semantics)
        state, prev, rows = _tiled(st[:n]), _tiled(pv[:n]), _rows(st, n, False)
        want = eng.step_wrench_tiled(state, n, DT, prev=prev)
        eng.set_prev_velocity(pv[:n])
        want_own = eng.step_wrench_tiled(state, n, DT)
        eng.set_prev_velocity(pv[:n])
        want_f, want_t = (x.clone() for x in eng.step_wrench_aos(*rows, DT))
        assert _same_bits(want_own, want)
        for sea in (None, still, flat):
            eng.set_sea(sea)
            for time in (0.0, 0.7):
                assert _same_bits(eng.step_wrench_tiled_sea(state, n, DT, time, prev=prev), want), (n, time)
                eng.set_prev_velocity(pv[:n])
                assert _same_bits(eng.step_wrench_tiled_sea(state, n, DT, time), want), (n, time)
                assert _prev_is(eng, st[:n, 7:13])
                eng.set_prev_velocity(pv[:n])
                f, t = eng.step_wrench_aos_sea(*rows, DT, time)
                assert _same_bits(f, want_f) and _same_bits(t, want_t), (n, time)
                assert _prev_is(eng, st[:n, 7:13])
        eng.close()


# ---- 6. refusals and guards, through the raw C ABI ---------------------------------------------------------------------------------------
def _banded(n, pad=16):
    """A flat NaN buffer that holds n rows of 3 floats between two bands of `pad` floats; (buffer, address of the rows)."""
    buf = torch.full((pad + 3 * n + pad,), NAN, device=DEV)
    return buf, buf.data_ptr() + 4 * pad


def _band_rows(buf, n, pad=16):
    host = buf.cpu().numpy()
    return host[pad:pad + 3 * n].reshape(n, 3), np.concatenate([host[:pad], host[pad + 3 * n:]])


def test_refusals_launch_nothing_and_legal_launches_stay_inside(pop, native_built):
    st, pv, params, _, _ = pop
    n, tiles = 257, 5
    eng = _engine(n, params["f32"], "f32")
    lib, h, stream = eng._lib, eng._h, eng._stream(None)
    state, prev = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV)
    before = [b.cpu().numpy() for b in (state, prev)]
    wrench = torch.full((tiles * S_WR,), NAN, device=DEV)
    (fbuf, f_ptr), (tbuf, t_ptr) = _banded(n), _banded(n)
    pos, quat, vel = _rows(st, n, False)
    marker = np.ascontiguousarray(pv[:n][::-1])                   # what the engine's record holds: no refused call may touch it
    eng.set_prev_velocity(marker)

    def tiled(time=1.0, n_=n, s=state.data_ptr(), ss=S_IN, p=prev.data_ptr(), ps=S_PV, dt=DT, w=wrench.data_ptr(), ws=S_WR):
        return lib.hydro_step_wrench_tiled_sea(h, n_, s, ss, p, ps, dt, w, ws, time, stream)

    def aos(time=1.0, n_=n, p=pos.data_ptr(), q=quat.data_ptr(), v=vel.data_ptr(), dt=DT, f=f_ptr, t=t_ptr):
        return lib.hydro_step_wrench_aos_sea(h, n_, p, q, 0, v, dt, f, t, time, stream)

    bad_times = (float("nan"), float("inf"), float("-inf"), -1e-300, -1.0, float(2 ** 52 + 1), 1e300)
    for sea in (SEA, None):                                      # `time` is validated whether or not a sea is set
        eng.set_sea(sea)
        for time in bad_times:
            assert tiled(time) == E_ARG and b"time must be finite" in lib.hydro_last_error(h), time
            assert aos(time) == E_ARG and b"time must be finite" in lib.hydro_last_error(h), time
        # the time is looked at first
        assert tiled(-1.0, n_=n + 1) == E_ARG and b"time must be finite" in lib.hydro_last_error(h)
        assert aos(-1.0, dt=0.0) == E_ARG and b"time must be finite" in lib.hydro_last_error(h)
        # then the parents' refusals
        for kw in (dict(n_=n + 1), dict(n_=-1), dict(dt=0.0), dict(dt=float("nan")), dict(s=None), dict(w=None), dict(w=wrench.data_ptr() + 4),
                   dict(ws=6 * 64 - 4), dict(ss=13 * 64 + 2), dict(p=prev.data_ptr() + 8), dict(ps=6 * 64 - 4), dict(ws=1 << 24)):
            assert tiled(**kw) == E_ARG, kw
        for kw in (dict(n_=n + 1), dict(n_=(1 << 26) + 1), dict(dt=0.0), dict(p=None), dict(f=None), dict(t=None), dict(t=t_ptr + 4), dict(f=f_ptr + 8),
                   dict(v=vel.data_ptr() + 4)):
            assert aos(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(wrench).all() and torch.isnan(fbuf).all() and torch.isnan(tbuf).all()
    assert all(_untouched(b, was) for b, was in zip((state, prev), before)) and _prev_is(eng, marker)

    # the legal launches next to them: the largest time there is, the bodies' fields and nothing else
    eng.set_sea(SEA)
    for time in (float(2 ** 52), 0.0, 1.0):
        wrench.fill_(NAN); fbuf.fill_(NAN); tbuf.fill_(NAN)
        assert tiled(time) == 0
        eng.set_prev_velocity(pv[:n])
        assert aos(time) == 0
        torch.cuda.synchronize()
        got, rest = _unguard(wrench, n, 6, S_WR)
        (f, f_band), (t, t_band) = _band_rows(fbuf, n), _band_rows(tbuf, n)
        assert np.isfinite(got).all() and np.isnan(rest).all(), "a sentinel of the tiled wrench was read or overwritten"
        assert np.isfinite(f).all() and np.isfinite(t).all() and np.isnan(f_band).all() and np.isnan(t_band).all()
        assert all(_untouched(b, was) for b, was in zip((state, prev), before)), "a caller-owned prev: nothing is written but the wrench"
        assert _prev_is(eng, st[:n, 7:13])
        want = eng.step_wrench_tiled_sea(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n]))
        assert np.array_equal(got.view(np.uint32), scenes.from_tiled(want.cpu().numpy(), n).view(np.uint32))
        assert np.array_equal(np.concatenate([f, t], axis=1).view(np.uint32), got.view(np.uint32))
    eng.close()


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_captured_prepared_rows_step_replays_to_the_eager_bits(pop, native_built):
    st, pv, params, _, _ = pop
    n = 4097
    eng = _engine(n, params["f16"], "f16")
    eng.set_sea(SeaState((0.4, -0.1, 0.05)))                      # current only: a captured launch replays at a frozen time
    pos, quat, vel = _rows(st, n, False)
    f = torch.full((n, 3), NAN, device=DEV)
    t = torch.full((n, 3), NAN, device=DEV)
    step = eng.prepare_step_wrench_aos(pos, quat, vel, f, t)
    eng.set_prev_velocity(pv[:n])
    step(DT, None, 2.5)
    torch.cuda.synchronize()
    want_f, want_t = f.clone(), t.clone()
    still_f, _ = (x.clone() for x in eng.step_wrench_aos(pos, quat, vel, DT))      # (prev is now the true velocity: set it again below)
    f.fill_(NAN); t.fill_(NAN)
    stream = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            step(DT, stream, 2.5)
        torch.cuda.synchronize()
        assert torch.isnan(f).all()                               # capturing records, it does not execute
        eng.set_prev_velocity(pv[:n])
        g.replay()
        stream.synchronize()
    assert _same_bits(f, want_f) and _same_bits(t, want_t)
    assert not _same_bits(want_f, still_f)                        # and the current is in it
    eng.close()


# ---- 8. the plugin -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [True, "callbacks", False], ids=["scene", "callbacks", "per-prim"])
def test_plugin_applies_the_direct_call_at_its_clock(batched, native_built):
    hb.REGISTRY.clear()
    world, host, prims, behaviors = build_main_scene(batched)
    n = len(prims)
    behaviors[0].set_sea(SEA)
    for b in behaviors:
        b.on_play()
    # the second engine: the same rows, the same previous velocities, the times 0, dt0, dt0 + dt1
    rows = np.stack([b._param_row(float(world.masses[i])) for i, b in enumerate(behaviors)])
    direct = HydroEngine(n, DEV, behaviors[0]._rho, behaviors[0]._g)     # the scene scalars as the prims' float attributes hold them
    direct.set_params(rows)
    direct.set_sea(SEA)
    dts = (1.0 / 60.0, 0.02, 1.0 / 90.0)
    time = 0.0
    applied = lambda: (torch.stack([world.applied[p.path][0] for p in prims]), torch.stack([world.applied[p.path][1] for p in prims]))  # noqa: E731
    for k, dt in enumerate(dts):
        host.step(dt)
        want_f, want_t = direct.step_wrench_aos_sea(world.positions, world.orientations, world.velocities, dt, time)
        torch.cuda.synchronize()
        got_f, got_t = applied()
        assert _same_bits(got_f, want_f) and _same_bits(got_t, want_t), (k, time)
        time = time + dt
        world.velocities += 0.01 * torch.randn_like(world.velocities)          # "PhysX" moves the bodies
        world.positions += 0.01 * torch.randn_like(world.positions)
    assert behaviors[-1].sea_time == (dts[0] + dts[1]) + dts[2]
    # clearing the sea returns to the bits of step_wrench_aos
    behaviors[0].set_sea(None)
    host.step(dts[0])
    want_f, want_t = direct.step_wrench_aos(world.positions, world.orientations, world.velocities, dts[0])
    torch.cuda.synchronize()
    got_f, got_t = applied()
    assert _same_bits(got_f, want_f) and _same_bits(got_t, want_t)
    for b in behaviors:
        b.on_stop()
    direct.close()
    hb.REGISTRY.clear()


# ---- 9. the example ------------------------------------------------------------------------------------------------------------------------
def test_plugin_buoy_in_waves_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "plugin_buoy_in_waves.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    assert "largest |z - z_eq - eta| over 600 steps" in res.stdout and "drift:" in res.stdout
