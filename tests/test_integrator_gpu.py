"""Every integrating entry of the library against the fp64 step of oracle/integrator_oracle.py, field group by field
group (position, quaternion, velocity, angular velocity), body by body.

The reference step always takes the wrench the device integrated: the wrench passed in for hydro_integrate[_tiled], the
`wrench=` output of the same launch for hydro_step_fused_tiled[_ke], the wrench of hydro_step_wrench_tiled on the same
inputs for hydro_step_fused_tiled_multi (which has no wrench output; the fused kernels are bit-identical to wrench +
integrate, tests/test_closed_loop_gpu.py).  So these tests isolate the integrator; wrench parity is gated elsewhere
(tests/test_parity_gpu.py).  The implicit form's drag coefficients are integrator_oracle.drag_jacobian of the oracle's
components.

Bound: integrator_error_ulps <= STEP_ULP_BOUND on every body and group (the metric and the bound are those of the CPU test
tests/test_integrator_oracle.py, which shows that typical mistakes land 100x above it).  Each test prints its largest
error per group."""
import numpy as np
import pytest
import torch

import populations
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from resident_harness import B, DEV, DT, _engine, G, _guarded, _k, NAN, _report, RHO, _tiled, _unguard, _untouched

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257, 4097, 100003)


@pytest.fixture(scope="module")
def pop():
    """The designed population at the largest size, its parameters per coefficient format, and per (format,
    semantics) the oracle wrench (fp32, as a device would hand it over) and the components drag_jacobian needs."""
    st, pv, pr = populations.integrator_population(n=max(SIZES), seed=31)
    params = {"f32": pr, "f16": pr.copy()}
    params["f16"][:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    cache = {}

    def oracle(coeff, semantics="numba"):
        if (coeff, semantics) not in cache:
            f, t, comps = ho.step_wrench(st, pv, params[coeff], RHO, G, DT, semantics)
            cache[coeff, semantics] = (np.concatenate([f, t], axis=1).astype(np.float32), comps)
        return cache[coeff, semantics]
    return st, pv, params, oracle


def _soa(x):
    return torch.from_numpy(scenes.to_soa(x)).to(DEV)


def _errors(got, st, wrench, params, k=None):
    ref = io.integrate(st, wrench, params, G, DT, *(k or (None, None)))
    err = io.integrator_error_ulps(got, ref, st, wrench, params, G, DT, k)
    return {g: float(np.nan_to_num(e, nan=np.inf).max(initial=0.0)) for g, e in err.items()}


# ------------------------------------------------------------------------------------------------------------ entries
@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_integrate_plain_soa_and_in_place(coeff, pop, native_built):
    """hydro_integrate on plain SoA, out of place and in place (state_out = state_in, which hydro.h allows)."""
    st, _, params, oracle = pop
    wrench, _ = oracle(coeff)
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        S, W = _soa(st[:n]), _soa(wrench[:n])
        out = eng.integrate(S, W, DT)
        inplace = S.clone()
        eng.integrate(inplace, W, DT, state_out=inplace)
        torch.cuda.synchronize()
        assert torch.equal(out, inplace), n
        worst[n] = _errors(out.cpu().numpy().T, st[:n], wrench[:n], pr[:n])
        eng.close()
    _report(f"integrate {coeff}", worst)


@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_integrate_tiled(coeff, pop, native_built):
    st, _, params, oracle = pop
    wrench, _ = oracle(coeff)
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        out = eng.integrate_tiled(_tiled(st[:n]), _tiled(wrench[:n]), n, DT)
        torch.cuda.synchronize()
        worst[n] = _errors(scenes.from_tiled(out.cpu().numpy(), n), st[:n], wrench[:n], pr[:n])
        eng.close()
    _report(f"integrate_tiled {coeff}", worst)


@pytest.mark.parametrize("coeff", ["f32", "f16"])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("ke", [False, True], ids=["", "ke"])
def test_step_fused_tiled(coeff, implicit, ke, pop, native_built):
    """hydro_step_fused_tiled[_ke] with the default ping-pong of the engine: the new state goes into the buffer the
    previous velocity is read from (state_out aliases prev_state)."""
    st, pv, params, oracle = pop
    _, comps = oracle(coeff)
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        old = np.zeros((n, 13), np.float32)
        old[:, 7:13] = pv[:n]
        cur, prev_state = _tiled(st[:n]), _tiled(old)
        w = eng.alloc_tiled(6, n)
        ke_out = torch.full((2,), NAN, dtype=torch.float64, device=DEV) if ke else None
        out = eng.step_fused_tiled(cur, prev_state, n, DT, wrench=w, implicit_drag=implicit, ke_out=ke_out)
        torch.cuda.synchronize()
        assert out.data_ptr() == prev_state.data_ptr()
        got = scenes.from_tiled(out.cpu().numpy(), n)
        used = scenes.from_tiled(w.cpu().numpy(), n)
        k = _k(comps, st, pr, coeff, n) if implicit else None
        worst[n] = _errors(got, st[:n], used, pr[:n], k)
        if ke:
            want = scenes.kinetic_energy_fp64(got, pr[:n])
            assert ke_out[0].item() == pytest.approx(want[0], rel=1e-12) and ke_out[1].item() == pytest.approx(want[1], rel=1e-12)
        eng.close()
    _report(f"step_fused_tiled{'_ke' if ke else ''} {'implicit' if implicit else 'explicit'} {coeff}", worst)


@pytest.mark.parametrize("coeff", ["f32", "f16"])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_step_fused_tiled_multi_one_step(coeff, implicit, pop, native_built):
    """hydro_step_fused_tiled_multi with steps = 1, through the engine's two-buffer ping-pong: the new state goes into
    the previous-state buffer and the velocity of the step before (the input's) into the velocity fields of `state`."""
    st, pv, params, oracle = pop
    _, comps = oracle(coeff)
    pr = params[coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        old = np.zeros((n, 13), np.float32)
        old[:, 7:13] = pv[:n]
        cur, prev_state = _tiled(st[:n]), _tiled(old)
        used = eng.step_wrench_tiled(cur, n, DT, prev=prev_state)            # the wrench the multi-step kernel integrates
        out = eng.step_fused_tiled_multi(cur, prev_state, n, DT, 1, implicit_drag=implicit)
        torch.cuda.synchronize()
        got = scenes.from_tiled(out.cpu().numpy(), n)
        assert np.array_equal(scenes.from_tiled(cur.cpu().numpy(), n), st[:n])      # prev_out: the velocity it started from
        k = _k(comps, st, pr, coeff, n) if implicit else None
        worst[n] = _errors(got, st[:n], scenes.from_tiled(used.cpu().numpy(), n), pr[:n], k)
        eng.close()
    _report(f"step_fused_tiled_multi(1) {'implicit' if implicit else 'explicit'} {coeff}", worst)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_step_fused_tiled_warp_semantics(implicit, pop, native_built):
    """HYDRO_SEM_WARP changes the wrench (added mass), not the integrator: same bound, with the k of the Warp twin's
    clamp."""
    st, pv, params, oracle = pop
    _, comps = oracle("f32", "warp")
    pr = params["f32"]
    n = 4097
    eng = _engine(n, pr, "f32", "warp")
    old = np.zeros((n, 13), np.float32)
    old[:, 7:13] = pv[:n]
    cur, prev_state = _tiled(st[:n]), _tiled(old)
    w = eng.alloc_tiled(6, n)
    out = eng.step_fused_tiled(cur, prev_state, n, DT, wrench=w, implicit_drag=implicit)
    torch.cuda.synchronize()
    k = _k(comps, st, pr, "f32", n) if implicit else None
    err = _errors(scenes.from_tiled(out.cpu().numpy(), n), st[:n], scenes.from_tiled(w.cpu().numpy(), n), pr[:n], k)
    eng.close()
    _report(f"step_fused_tiled warp {'implicit' if implicit else 'explicit'} f32", {n: err})


# ------------------------------------------------------------------------------- strides and guard regions (C ABI)


@pytest.mark.parametrize("entry", ["integrate_tiled", "fused", "fused_ke", "multi"])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_tiled_entries_with_strides_and_nan_guards(entry, implicit, coeff, pop, native_built):
    """Straight through the C ABI: tile strides larger than F * 64 and different for every buffer, NaN in the stride
    padding and past body n of every buffer.  The outputs of the bodies are the fp64 step's (no sentinel read), and no
    sentinel is overwritten."""
    if entry == "integrate_tiled" and implicit:
        pytest.skip("hydro_integrate_tiled has no implicit form")
    st, pv, params, oracle = pop
    wrench_in, comps = oracle(coeff)
    pr = params[coeff]
    S_IN, S_OUT, S_W, S_PV, S_PVO = 13 * 64 + 36, 13 * 64 + 100, 6 * 64 + 8, 6 * 64 + 20, 6 * 64 + 12
    worst = {}
    for n in (65, 4097):
        eng = _engine(n, pr, coeff)
        lib, h, stream = eng._lib, eng._h, eng._stream(None)
        state = _guarded(st[:n], S_IN)
        out = torch.full(((n + 63) // 64 * S_OUT,), NAN, device=DEV)
        state_before = state.cpu().numpy()
        if entry == "integrate_tiled":
            wbuf = _guarded(wrench_in[:n], S_W)
            w_before = wbuf.cpu().numpy()
            rc = lib.hydro_integrate_tiled(h, n, state.data_ptr(), S_IN, wbuf.data_ptr(), S_W, DT, out.data_ptr(), S_OUT, stream)
        else:
            prev = _guarded(pv[:n], S_PV)
            pv_before = prev.cpu().numpy()
            if entry == "multi":
                pvo = torch.full(((n + 63) // 64 * S_PVO,), NAN, device=DEV)
                rc = lib.hydro_step_fused_tiled_multi(h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT, 1,
                                                      out.data_ptr(), S_OUT, pvo.data_ptr(), S_PVO, int(implicit), 1, None, stream)
                wbuf = _guarded(np.zeros((n, 6), np.float32), S_W)
                eng._check(lib.hydro_step_wrench_tiled(h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT,
                                                       wbuf.data_ptr(), S_W, stream))
            else:
                wbuf = torch.full(((n + 63) // 64 * S_W,), NAN, device=DEV)
                if entry == "fused":
                    rc = lib.hydro_step_fused_tiled(h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT, out.data_ptr(), S_OUT,
                                                    wbuf.data_ptr(), S_W, int(implicit), stream)
                else:
                    ke_out = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
                    rc = lib.hydro_step_fused_tiled_ke(h, n, state.data_ptr(), S_IN, prev.data_ptr(), S_PV, DT, out.data_ptr(), S_OUT,
                                                       wbuf.data_ptr(), S_W, int(implicit), 1, ke_out.data_ptr(), stream)
        eng._check(rc)
        torch.cuda.synchronize()
        got, rest = _unguard(out, n, 13, S_OUT)
        assert np.isnan(rest).all(), (entry, n, "a sentinel of state_out was overwritten")
        assert _untouched(state, state_before)
        if entry == "integrate_tiled":
            used = wrench_in[:n]
            assert _untouched(wbuf, w_before)
        else:
            assert _untouched(prev, pv_before)
            used, wrest = _unguard(wbuf, n, 6, S_W)
            if entry != "multi":
                assert np.isnan(wrest).all(), (entry, n, "a sentinel of the wrench output was overwritten")
            else:
                pv_out, prest = _unguard(pvo, n, 6, S_PVO)
                assert np.isnan(prest).all() and np.array_equal(pv_out, st[:n, 7:13])
        assert np.isfinite(got).all() and np.isfinite(used).all(), (entry, n, "a sentinel was read")
        if entry == "fused_ke":
            want = scenes.kinetic_energy_fp64(got, pr[:n])
            assert ke_out[0].item() == pytest.approx(want[0], rel=1e-12) and ke_out[1].item() == pytest.approx(want[1], rel=1e-12)
        k = _k(comps, st, pr, coeff, n) if implicit else None
        worst[n] = _errors(got, st[:n], used, pr[:n], k)
        eng.close()
    _report(f"C ABI {entry} {'implicit' if implicit else 'explicit'} {coeff}, strides {S_IN}/{S_OUT}", worst)


# ------------------------------------------------------------------------------------------ multi-step trajectories
# Largest error after k resident steps against the fp64 closed loop, in units of ULP * the running scale after step k:
# about 4x the largest value measured on the MI355X over the three scenes, which was 3.8 / 165 / 123 / 349 / 433 / 1604
# after 1 / 2 / 4 / 8 / 16 / 32 steps (C2 alone: 2.0 / 2.7 / 9.0 / 10.1 / 32.2 / 80.2; C3: 2.9 / 13.6 / 43.4 / 38.7 / 93.7
# / 102.5; the population carries the rest).
TRAJECTORY_STEPS = (1, 2, 4, 8, 16, 32)
TRAJECTORY_BOUND = {1: B, 2: 660.0, 4: 660.0, 8: 1400.0, 16: 1800.0, 32: 6400.0}
# A body is ill-conditioned when its fp64 loop, started from the same state moved by one fp32 ulp, is this far (same
# units) from the unmoved one after k steps.
ILL_CONDITIONED = {1: 6.0, 2: 30.0, 4: 45.0, 8: 175.0, 16: 200.0, 32: 200.0}
# measured exclusions (branch margin + ill-conditioned): C2 513 / 4096, C3 281 / 19456, population 610 / 2266 - the
# population's thin slabs spinning at up to 10 rad/s tumble, which no fixed-step loop follows to fp32 precision
EXCLUDED_MAX = {"c2": 0.15, "c3": 0.02, "population": 0.3}


def _trajectory_scene(name):
    if name == "c2":
        return scenes.scene_c2(), False
    if name == "c3":
        return scenes.scene_c3(), True
    st, pv, pr = populations.integrator_population(n=24000, seed=33)
    # The added mass acts on the finite-difference acceleration of the previous step, explicitly: a fixed-step loop holds
    # it only while the added mass is below the body's own (v' - v = -(A / m)(v - v_prev) + ...).  The implicit form
    # treats the drag, not that; keep the bodies on which the loop is defined.
    p = pr.astype(np.float64)
    wet_mass = RHO * p[:, 0] * p[:, 1] * p[:, 2]
    keep = (wet_mass * p[:, 8] < 0.5 * p[:, 10]) & (12.0 * wet_mass * p[:, 9] < 0.5 * p[:, 10])
    # Where the drag takes a body nearly to rest within one step (|k| dt / m >> 1), the next step's drag coefficients
    # depend on |v'| and |w'|, which are then the rounding residue of the first step: that trajectory is not determined
    # to fp32 precision by anything (measured: 2 ulps on the first step's velocity change the second by 1e6 ulps).  Those
    # bodies are what the single-step tests above cover; the trajectory keeps |k| dt / m and |k| dt / I below 2.
    _, _, comps = ho.step_wrench(st, pv, pr, RHO, G, DT)
    kl, ka = io.drag_jacobian(st, pr, comps, RHO)
    keep &= (np.abs(kl) * DT < 2.0 * p[:, 10]) & (np.abs(ka) * DT < 2.0 * io.box_inertia(pr).min(axis=1))
    return scenes.Scene("integrator population", st[keep], pv[keep], pr[keep], RHO, G, DT), True


def _ill_conditioned(sc, implicit, ref, scales):
    """Bodies whose fp64 closed loop is not determined to fp32 precision by its start: the same loop from the start
    state moved by one fp32 ulp in every field leaves ILL_CONDITIONED at some checkpoint."""
    rng = np.random.default_rng(7)
    moved = np.where(rng.integers(0, 2, sc.state.shape) == 1, np.nextafter(sc.state, np.float32(np.inf)),
                     np.nextafter(sc.state, np.float32(-np.inf))).astype(np.float32)
    alt = io.closed_loop(moved, sc.prev, sc.params, sc.rho, sc.g, sc.dt, max(TRAJECTORY_STEPS), implicit)
    bad = np.zeros(sc.n, bool)
    for k in TRAJECTORY_STEPS:
        r = ref[k - 1]
        err = io.integrator_error_ulps(alt[k - 1]["state"], r["state"], r["input"], r["wrench"], sc.params, sc.g, sc.dt,
                                       scales=scales[k - 1])
        bad |= np.max(np.stack([np.nan_to_num(e, nan=np.inf) for e in err.values()]), axis=0) > ILL_CONDITIONED[k]
    return bad


@pytest.mark.parametrize("name", ["c2", "c3", "population"])
def test_resident_trajectory_follows_the_fp64_closed_loop(name, native_built):
    """32 steps of ClosedLoopSim.run_resident (C2 explicit; C3 and the designed population implicit) against the fp64
    closed loop of integrator_oracle.closed_loop (oracle wrench, `integrate`, the state rounded to fp32 after every step
    as the device stores it), read after 1, 2, 4, 8, 16 and 32 steps.  The two loops start from the same fp32 state and
    drift apart by rounding: the error is measured against the largest scales of the steps so far
    (integrator_oracle.running_scales) and the bound grows with the step count (TRAJECTORY_BOUND).
    Left out: bodies whose reference state comes within a branch margin of 1e-4 (scenes.branch_margins) at any step -
    there the two loops may take different branches of the model - and bodies whose fp64 loop is itself not determined
    to fp32 precision (_ill_conditioned).  Over 32 steps the first is not the 1 % of a single step: bobbing buoys carry
    27 keypoints and 6 face centres through the surface, and a keypoint that passes within 1e-4 L of it is an exclusion
    (C2: 12 %, C3: 1.4 %, the population: 10 %, measured on the fp64 loop); EXCLUDED_MAX caps the total per scene."""
    sc, implicit = _trajectory_scene(name)
    ref = io.closed_loop(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt, max(TRAJECTORY_STEPS), implicit)
    margin = np.minimum.accumulate(np.stack([r["margin"] for r in ref]), axis=0)
    scales = io.running_scales(ref, sc.params, sc.g, sc.dt)
    ill = _ill_conditioned(sc, implicit, ref, scales)
    sim = ClosedLoopSim(sc, implicit_drag=implicit)
    done, measured = 0, {}
    for k in TRAJECTORY_STEPS:
        sim.run_resident(k - done)
        done = k
        got = sim.state()
        r = ref[k - 1]
        keep = (margin[k - 1] >= 1e-4) & ~ill
        err = io.integrator_error_ulps(got[keep], r["state"][keep], r["input"][keep], r["wrench"][keep], sc.params[keep],
                                       sc.g, sc.dt, scales={g: v[keep] for g, v in scales[k - 1].items()})
        measured[k] = {g: float(np.nan_to_num(e, nan=np.inf).max(initial=0.0)) for g, e in err.items()}
    sim.close()
    near = int((margin[-1] < 1e-4).sum())
    print(f"[trajectory {name}] {sc.n} bodies, {near} excluded by the branch margin, {int((ill & (margin[-1] >= 1e-4)).sum())} "
          f"more as ill-conditioned; max ulps after k steps: "
          + "; ".join(f"{k}: " + " ".join(f"{g[:4]} {v:.1f}" for g, v in m.items()) for k, m in measured.items()))
    assert (~keep).sum() <= EXCLUDED_MAX[name] * sc.n
    bad = {k: m for k, m in measured.items() if max(m.values()) > TRAJECTORY_BOUND[k]}
    assert not bad, (name, bad)
