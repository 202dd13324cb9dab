"""Parity tests proper: the HIP path, called through the C ABI, against the fp64 oracle.

Gate (north_star: "per-body wrench parity to the Numba reference within 1e-5 relative"):
    max( |dF| / max(|F_ref|, 1e-3 rho g V),  |dT| / max(|T_ref|, 1e-3 rho g V L) ) <= 1e-5
per body, on the golden fixtures (whose reference outputs came from the
reference itself) and on seeded scenes.  At BASELINE's full sizes the oracle would be slow, so
size-independent properties are used there (exact zeros for dry bodies, x/y translation
invariance, sharded == unsharded bit for bit, yaw equivariance)."""
import numpy as np
import pytest
import torch

from conftest import SCENE_FIXTURES, accel_of, load_golden
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd._native import HydroError
from silver2_isaacsim_amd.engine import HydroEngine

pytestmark = pytest.mark.gpu
GATE = 1e-5
DEV = "cuda:0"


def soa(x):
    return torch.from_numpy(scenes.to_soa(x)).to(DEV)


def run_ext(state, prev, params, rho, g, dt, coeff="f32", vec=0, block=0, nt=-1):
    eng = HydroEngine(len(state), DEV, rho, g)
    eng.set_params(params, coeff)
    eng.set_tuning(vec, block, nt)
    out = eng.step_wrench(soa(state), dt, prev=soa(prev))
    torch.cuda.synchronize()
    eng.close()
    o = out.cpu().numpy().T
    return o[:, :3], o[:, 3:]


@pytest.mark.parametrize("name", SCENE_FIXTURES)
@pytest.mark.parametrize("vec", [1, 2])
def test_fused_wrench_matches_oracle_on_fixtures(name, vec, native_built):
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    coeff = "f16" if name == "c5" else "f32"
    f, t = run_ext(fx["state"], fx["prev"], fx["params"], rho, g, dt, coeff, vec)
    rf, rt, aux = ho.step_wrench(fx["state"], fx["prev"], fx["params"], rho, g, dt)
    err = ho.wrench_error(f, t, rf, rt, fx["params"], rho, g)
    assert np.isfinite(f).all() and np.isfinite(t).all()
    assert err.max() <= GATE, f"{name} vec={vec}: {err.max():.3e}"
    # ... and directly against what the reference's own _apply_behavior produced (fixture)
    assert ho.wrench_error(f, t, fx["net_force"], fx["net_torque"], fx["params"], rho, g).max() <= GATE
    dry = aux["ratio"] == 0.0
    assert np.all(f[dry] == 0.0) and np.all(t[dry] == 0.0)


@pytest.mark.parametrize("dt", [1.0 / 60.0, 1.0 / 120.0, 0.004999999999999999])
def test_dt_is_a_double_through_the_abi(dt, native_built):
    """The reference's callback receives `delta_time` as a Python float (hydrodynamics_behavior.py:138); the parity
    target - the Numba / fp64 oracle - evaluates the finite difference (v - v_last) / dt in float64.  (The shipped
    behaviour itself divides fp32 torch tensors and feeds the fp32 Warp calculator, :200-209: the fp64 target is this
    repository's oracle of the Numba path, not that pipeline.)  1/60 is not an fp32 number: rounded to fp32 it is 5e-8
    off, which an added-mass-dominated body shows in full.  The C ABI takes dt as a double; results follow the oracle
    evaluated with the SAME double to fp32 rounding, and differ from those of the fp32-rounded step."""
    sc = scenes.scene_c2()
    params = sc.params.copy()
    params[:, 8] *= 20.0; params[:, 9] *= 20.0                       # added mass dominates the wrench
    f, t = run_ext(sc.state, sc.prev, params, sc.rho, sc.g, dt)
    rf, rt, _ = ho.step_wrench(sc.state, sc.prev, params, sc.rho, sc.g, dt)
    err = ho.wrench_error(f, t, rf, rt, params, sc.rho, sc.g)
    assert err.max() <= 3e-7, err.max()
    rf32, rt32, _ = ho.step_wrench(sc.state, sc.prev, params, sc.rho, sc.g, float(np.float32(dt)))
    err32 = ho.wrench_error(f, t, rf32, rt32, params, sc.rho, sc.g)
    assert err32.max() > err.max()                                   # the rounded step is a different (worse) answer


@pytest.mark.parametrize("name,builder", [("C2", scenes.scene_c2), ("C3", scenes.scene_c3)])
def test_full_config_gate(name, builder, native_built):
    """Configs 2 and 3 in full (4 096 buoys; 19 x 1 024 hexapod links): gate 1e-5 on every body."""
    sc = builder()
    f, t = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    rf, rt, _ = ho.step_wrench(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    err = ho.wrench_error(f, t, rf, rt, sc.params, sc.rho, sc.g)
    assert err.max() <= GATE


def test_ungated_population_report(native_built):
    """No branch-margin rule (adversarial set): with every branch of the model decided on fp64
    quantities, like the reference's, this set needs no allowance either."""
    sc = scenes.scene_c4(n=131072, seed=4242, margin=None)
    f, t = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    rf, rt, _ = ho.step_wrench(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    err = ho.wrench_error(f, t, rf, rt, sc.params, sc.rho, sc.g)
    print(f"ungated 131072 bodies: max {err.max():.3e} p99.9 {np.percentile(err, 99.9):.3e} n>1e-5 {(err > GATE).sum()}")
    assert err.max() <= 5e-7


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 257, 1000, 4095])
@pytest.mark.parametrize("vec", [1, 2])
def test_ragged_sizes(n, vec, native_built):
    fx = load_golden("c4")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    st, pv, pr = fx["state"][:n], fx["prev"][:n], fx["params"][:n]
    f, t = run_ext(st, pv, pr, rho, g, dt, vec=vec)
    f1, t1 = run_ext(fx["state"], fx["prev"], fx["params"], rho, g, dt, vec=1)
    assert np.array_equal(f, f1[:n]) and np.array_equal(t, t1[:n])          # same bits as the big launch


@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_every_launch_geometry_gives_the_same_bits(coeff, native_built):
    """bodies/lane x block size x (non-)temporal accesses: tuning must never change a result."""
    fx = load_golden("c5")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = 2047                                      # odd: exercises the remainder launch of vec=2
    ref = None
    for vec in (1, 2):
        for block in (128, 256):
            for nt in (0, 1):
                f, t = run_ext(fx["state"][:n], fx["prev"][:n], fx["params"][:n], rho, g, dt, coeff, vec, block, nt)
                if ref is None:
                    ref = (f, t)
                assert np.array_equal(f, ref[0]) and np.array_equal(t, ref[1]), (vec, block, nt)


def test_output_tail_is_not_touched(native_built):
    """A launch over n bodies must not write past element n of any output field."""
    fx = load_golden("c2")
    n = 1001
    eng = HydroEngine(2048, DEV, float(fx["rho"]), float(fx["g"]))
    eng.set_params(fx["params"][:2048])
    out = torch.full((6, 2048), -777.0, device=DEV)
    S, P = soa(fx["state"][:2048]), soa(fx["prev"][:2048])
    for vec in (1, 2):
        out.fill_(-777.0)
        eng.set_tuning(vec)
        lib_n = eng._lib.hydro_step_wrench_ext(eng._h, n, eng._table(S, 13), eng._table(P, 6), float(fx["dt"]),
                                               eng._table(out, 6), eng._stream(None))
        assert lib_n == 0
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.all(o[:, n:] == -777.0) and np.all(o[:, :n] != -777.0)
    eng.close()


def test_engine_owned_previous_velocity(native_built):
    fx = load_golden("c4")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = len(fx["state"])
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(fx["params"])
    S = soa(fx["state"])
    # first step: previous velocity is zero (hydrodynamics_behavior.py:196-198)
    out0 = eng.step_wrench(S, dt).cpu().numpy().T
    rf, rt, _ = ho.step_wrench(fx["state"], np.zeros_like(fx["prev"]), fx["params"], rho, g, dt)
    assert ho.wrench_error(out0[:, :3], out0[:, 3:], rf, rt, fx["params"], rho, g).max() <= GATE
    # ... and the engine now holds this step's velocity, exactly (:237-238)
    assert np.array_equal(eng.get_prev_velocity().cpu().numpy().T, fx["state"][:, 7:13])
    # checkpoint / resume of the only persistent state
    eng.set_prev_velocity(fx["prev"])
    out1 = eng.step_wrench(S, dt).cpu().numpy().T
    f, t = run_ext(fx["state"], fx["prev"], fx["params"], rho, g, dt)
    assert np.array_equal(out1[:, :3], f) and np.array_equal(out1[:, 3:], t)
    eng.reset_prev_velocity()
    assert float(eng.get_prev_velocity().abs().max()) == 0.0
    eng.close()


@pytest.mark.parametrize("name", ["c2", "c4", "c5"])
def test_array_of_structs_entry(name, native_built):
    """The simulator-facing entry (wxyz quaternions, (N,3)/(N,4)/(N,6) tensors, LDS transposition)."""
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    st = fx["state"]
    for n in (len(st), 777, 1):
        eng = HydroEngine(n, DEV, rho, g)
        eng.set_params(fx["params"][:n], "f16" if name == "c5" else "f32")
        eng.set_prev_velocity(fx["prev"][:n])
        pos = torch.from_numpy(np.ascontiguousarray(st[:n, 0:3])).to(DEV)
        q_wxyz = torch.from_numpy(np.ascontiguousarray(st[:n, [6, 3, 4, 5]])).to(DEV)
        vel = torch.from_numpy(np.ascontiguousarray(st[:n, 7:13])).to(DEV)
        F, T = eng.step_wrench_aos(pos, q_wxyz, vel, dt)
        torch.cuda.synchronize()
        rf, rt, _ = ho.step_wrench(st[:n], fx["prev"][:n], fx["params"][:n], rho, g, dt)
        err = ho.wrench_error(F.cpu().numpy(), T.cpu().numpy(), rf, rt, fx["params"][:n], rho, g)
        assert err.max() <= GATE
        assert np.array_equal(eng.get_prev_velocity().cpu().numpy().T, st[:n, 7:13])
        # xyzw order gives the same bits
        eng.set_prev_velocity(fx["prev"][:n])
        q_xyzw = torch.from_numpy(np.ascontiguousarray(st[:n, 3:7])).to(DEV)
        F2, T2 = eng.step_wrench_aos(pos, q_xyzw, vel, dt, quat_xyzw=True)
        assert torch.equal(F, F2) and torch.equal(T, T2)
        eng.close()


@pytest.mark.parametrize("name", ["kat", "c2", "c4"])
def test_component_mode_matches_reference_outputs(name, native_built):
    """Eight component vectors + ratio against the reference's own outputs (fixtures)."""
    fx = load_golden(name)
    rho, g = float(fx["rho"]), float(fx["g"])
    n = len(fx["state"])
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(fx["params"])
    comps, ratio = eng.step_components(soa(fx["state"]), soa(accel_of(fx).astype(np.float32)))
    torch.cuda.synchronize()
    eng.close()
    c = comps.cpu().numpy().T.reshape(n, 8, 3)
    ref = fx["components"]
    vol = fx["params"][:, :3].astype(np.float64).prod(1)
    floor = np.maximum(1e-3 * rho * g * vol, 1e-12)[:, None]
    rel = np.linalg.norm(c[:, :6] - ref[:, :6], axis=2) / np.maximum(np.linalg.norm(ref[:, :6], axis=2), floor)
    cen = np.abs(c[:, 6:] - ref[:, 6:]).max()
    ulp_p = np.spacing(np.float32(np.abs(fx["state"][:, :3]).max() + 2.0))     # centres are world-space fp32 numbers
    print(f"[components {name}] per-component max {rel.max():.3e} median {np.median(rel):.3e}; centres max {cen:.3e} m (fp32 ulp there {ulp_p:.3e})")
    # the body is evaluated in fp64 and each component rounded to fp32 ONCE: half an ulp per coordinate, i.e. at most
    # sqrt(3) * 2^-24 = 1.03e-7 of the component's own norm (a bound, not an allowance; was 5e-5 for the fp32 body).
    # On top of that this entry takes the ACCELERATIONS as fp32 arrays while the fixtures' reference outputs used the
    # float64 finite difference: the added-mass components (linear in the acceleration) inherit that input rounding,
    # another 1.03e-7 -> 2.1e-7 in all (measured: c2 1.09e-7, c4 1.86e-7).
    # The K vectors ("kat") are the exception: their inputs are float64 numbers (SURVEY's raw quaternions normalised in
    # fp64), so handing them to an fp32 interface rounds the INPUTS by 6e-8 and the lift follows with 5e-7.
    assert rel.max() < (2.1e-7 if name != "kat" else 2e-6)
    assert np.median(rel) < 6e-8
    # centres: fp64 lever arm + position, rounded once to a world-space fp32 number: half an ulp of |p|
    assert cen <= 0.5 * ulp_p * 1.0001
    assert np.abs(ratio.cpu().numpy() - fx["ratio"]).max() < 5e-7
    dry = fx["ratio"] == 0
    assert np.all(c[dry] == 0.0)                  # Numba semantics: cob = cop = 0 when dry (N6)


def test_prepared_step_is_the_same_launch(native_built):
    """prepare_step_wrench_tiled: arguments validated once, the callable re-issues the launch (same bits),
    follows the buffers' contents, and refuses to run on a closed engine."""
    fx = load_golden("c2")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = 1000
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(fx["params"][:n])
    S, P = tiled(fx["state"][:n]), tiled(fx["prev"][:n])
    ref = eng.step_wrench_tiled(S, n, dt, prev=P).clone()
    out = eng.alloc_tiled(6, n)
    step = eng.prepare_step_wrench_tiled(S, n, dt, out=out, prev=P)
    assert step() is out
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    S[:, 2, :] -= 0.25                                   # same buffers, new contents
    step(); ref2 = eng.step_wrench_tiled(S, n, dt, prev=P)
    torch.cuda.synchronize()
    assert torch.equal(out, ref2) and not torch.equal(out, ref)
    with pytest.raises(ValueError):
        eng.prepare_step_wrench_tiled(S[:, :5], n, dt)   # wrong field count is caught at prepare time
    eng.close()
    with pytest.raises(HydroError, match="HYDRO_E_STATE"):
        step()


def test_error_statuses(native_built):
    fx = load_golden("c2")
    eng = HydroEngine(128, DEV)
    S = soa(fx["state"][:256]); P = soa(fx["prev"][:256])
    with pytest.raises(HydroError, match="HYDRO_E_STATE"):          # step before set_params
        eng.step_wrench(S[:, :128].contiguous(), 1 / 60)
    eng.set_params(fx["params"][:128])
    with pytest.raises(HydroError, match="HYDRO_E_ARG"):            # n > capacity
        eng.step_wrench(S, 1 / 60, prev=P)
    with pytest.raises(HydroError, match="HYDRO_E_ARG"):            # dt <= 0
        eng.step_wrench(S[:, :128].contiguous(), 0.0)
    with pytest.raises(HydroError, match="HYDRO_E_ARG"):
        eng.set_tuning(3)
    with pytest.raises(HydroError, match="HYDRO_E_ARG"):
        eng.set_tuning(0, 0, -1, 9)
    with pytest.raises(ValueError):
        eng.set_semantics("cuda")
    assert eng._lib.hydro_set_semantics(eng._h, 7) == -1 and b"semantics" in eng._lib.hydro_last_error(eng._h)
    assert isinstance(HydroError(-1, "x"), RuntimeError)            # the plugin's except clause catches it
    with pytest.raises(HydroError, match="HYDRO_E_DEVICE"):
        HydroEngine(16, "cuda:63")
    # small accessors
    import ctypes
    cnt = ctypes.c_int(-1)
    assert eng._lib.hydro_device_count(ctypes.byref(cnt)) == 0 and cnt.value == torch.cuda.device_count()
    assert eng._lib.hydro_stream(eng._h) and eng._lib.hydro_stream(None) is None      # the engine's private copy stream
    assert eng._lib.hydro_capacity(eng._h) == 128
    # n == 0 is a no-op, not an error
    empty = torch.empty((13, 0), device=DEV)
    assert eng.step_wrench(empty, 1 / 60).shape == (6, 0)
    eng.close()
    with pytest.raises(ValueError):
        HydroEngine(16, "cpu")


def test_kinetic_energy_reduction(native_built):
    sc = scenes.scene_c4(n=100003, seed=5)
    eng = HydroEngine(sc.n, DEV, sc.rho, sc.g)
    eng.set_params(sc.params)
    S = soa(sc.state)
    a = eng.kinetic_energy(S, rotational=True).cpu().numpy()
    b = eng.kinetic_energy(S, rotational=True).cpu().numpy()
    assert np.array_equal(a, b)                                       # deterministic (no atomics)
    lin = ho.kinetic_energy(sc.state, sc.params, False)[0]
    tot = ho.kinetic_energy(sc.state, sc.params, True)[0]
    assert a[0] == pytest.approx(lin, rel=1e-12)                      # fp64 accumulation of exact fp32 products
    assert a.sum() == pytest.approx(tot, rel=1e-12)                   # the rotational term is fp64 per body as well
    only_lin = eng.kinetic_energy(S, rotational=False).cpu().numpy()
    assert only_lin[1] == 0.0 and only_lin[0] == a[0]
    t = eng.kinetic_energy(torch.from_numpy(scenes.to_tiled(sc.state)).to(DEV), rotational=True).cpu().numpy()
    assert np.array_equal(t, a)                                       # tiled layout: same bits
    eng.close()


@pytest.mark.parametrize("coeff", ["f32", "f16"])
@pytest.mark.parametrize("n", [100003, 257, 64, 1])
def test_kinetic_energy_sampled_inside_the_step_kernels(coeff, n, native_built):
    """SURVEY.md 8e "reduced in-kernel": hydro_step_wrench_tiled_ke / hydro_step_fused_tiled_ke sample the energy of
    the bodies they hold.  Same wrench / state bits as the plain kernels; the pair has the bits of the stand-alone
    reduction of the same state (same per-body arithmetic, same decomposition) and equals the fp64 host sum."""
    sc = scenes.scene_c4(n=n, seed=21)
    eng = HydroEngine(sc.n, DEV, sc.rho, sc.g)
    eng.set_params(sc.params, coeff)
    prm = sc.params.copy()
    if coeff == "f16":
        prm[:, 3:10] = prm[:, 3:10].astype(np.float16).astype(np.float32)
    st, pv = tiled(sc.state), tiled(sc.prev)
    plain = eng.step_wrench_tiled(st, sc.n, sc.dt, prev=pv)
    ke = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    sampled = eng.step_wrench_tiled(st, sc.n, sc.dt, prev=pv, ke_out=ke, rotational=True)
    alone = eng.kinetic_energy(st, rotational=True)
    torch.cuda.synchronize()
    assert torch.equal(plain, sampled)                                 # the wrench does not notice
    assert torch.equal(ke, alone)                                      # in-kernel sample == stand-alone reduction, bit for bit
    tot = ho.kinetic_energy(sc.state, prm, True)[0]; lin = ho.kinetic_energy(sc.state, prm, False)[0]
    assert ke[0].item() == pytest.approx(lin, rel=1e-12) and ke.sum().item() == pytest.approx(tot, rel=1e-12)
    ke_lin = torch.zeros(2, dtype=torch.float64, device=DEV)
    eng.step_wrench_tiled(st, sc.n, sc.dt, prev=pv, ke_out=ke_lin, rotational=False)
    torch.cuda.synchronize()
    assert ke_lin[0].item() == ke[0].item() and ke_lin[1].item() == 0.0
    # engine-owned previous velocity (the WRITE_PREV kernels) and the prepared form
    eng.set_prev_velocity(sc.prev); own = eng.step_wrench_tiled(st, sc.n, sc.dt)
    eng.set_prev_velocity(sc.prev); ke2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    own_s = eng.step_wrench_tiled(st, sc.n, sc.dt, ke_out=ke2)
    step = eng.prepare_step_wrench_tiled(st, sc.n, sc.dt, prev=pv, ke_out=torch.zeros(2, dtype=torch.float64, device=DEV))
    step()
    torch.cuda.synchronize()
    assert torch.equal(own, own_s) and torch.equal(ke2, ke) and torch.equal(own, plain)
    # the fused step samples the state it WRITES
    prev_state = np.zeros_like(sc.state); prev_state[:, 7:13] = sc.prev
    for implicit in (False, True):
        old_a, old_b = tiled(prev_state), tiled(prev_state)
        kf = torch.zeros(2, dtype=torch.float64, device=DEV)
        new_plain = eng.step_fused_tiled(st, old_a, sc.n, sc.dt, implicit_drag=implicit)
        new_sampled = eng.step_fused_tiled(st, old_b, sc.n, sc.dt, implicit_drag=implicit, ke_out=kf)
        alone_new = eng.kinetic_energy(new_plain, rotational=True)
        torch.cuda.synchronize()
        assert torch.equal(new_plain, new_sampled) and torch.equal(kf, alone_new)
        host_new = ho.kinetic_energy(scenes.from_tiled(new_plain.cpu().numpy(), sc.n), prm, True)[0]
        assert kf.sum().item() == pytest.approx(host_new, rel=1e-12)
    with pytest.raises(ValueError):
        eng.step_wrench_tiled(st, sc.n, sc.dt, prev=pv, ke_out=torch.zeros(2, device=DEV))     # float32: refused
    eng.close()


@pytest.mark.parametrize("n", [1048576 + 3, 4194304, 255, 1])
def test_kinetic_energy_single_launch_reduction_is_order_independent_and_replayable(n, native_built):
    """The reduction is one launch: the block that draws the last ticket adds the per-group pairs in a fixed order.  Which
    block that is varies from launch to launch; the bits must not (20 launches), the ticket counter must be back at zero
    after each (or the next launch would never finish its sum), a captured launch must replay, and the value is the
    fp64 host sum."""
    sc = scenes.scene_c4(n=min(n, 65536), seed=9)
    reps = -(-n // sc.n)
    state = np.tile(sc.state, (reps, 1))[:n]; params = np.tile(sc.params, (reps, 1))[:n]
    eng = HydroEngine(n, DEV, sc.rho, sc.g)
    eng.set_params(params)
    st = tiled(state)
    first = eng.kinetic_energy(st, rotational=True).clone()
    for _ in range(20):
        assert torch.equal(eng.kinetic_energy(st, rotational=True), first)
    tot = ho.kinetic_energy(state, params, True)[0]
    assert first.sum().item() == pytest.approx(tot, rel=1e-12)
    side = torch.cuda.Stream()
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        eng.kinetic_energy(st, rotational=True, out=out)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            eng.kinetic_energy(st, rotational=True, out=out)
    for _ in range(5):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
    # the sampling wrench kernel shares the scratch and the ticket: alternate the two
    prev = tiled(np.tile(sc.prev, (reps, 1))[:n])
    ke = torch.zeros(2, dtype=torch.float64, device=DEV)
    for _ in range(3):
        eng.step_wrench_tiled(st, n, sc.dt, prev=prev, ke_out=ke, rotational=True)
        assert torch.equal(eng.kinetic_energy(st, rotational=True), first)
        assert torch.equal(ke, first)
    eng.close()


def test_kinetic_energy_sees_every_update_of_the_state(native_built):
    """The reduction's partials and class sums cross blocks (and XCDs, each behind its own L2) through device-scope
    accesses within one launch.  A stale value anywhere would go unnoticed while the state stays the same from launch to
    launch - here it changes before every launch (300 launches, two sizes alternating on two engines), and every result
    must be the fp64 sum of THAT state to 1e-12."""
    sc = scenes.scene_c4(n=65536, seed=17)
    engines = []
    for n in (1048576, 300000):
        reps = -(-n // sc.n)
        state = np.tile(sc.state, (reps, 1))[:n]; params = np.tile(sc.params, (reps, 1))[:n]
        eng = HydroEngine(n, DEV, sc.rho, sc.g)
        eng.set_params(params)
        st = tiled(state)
        mass = torch.from_numpy(params[:, 10].astype(np.float64)).to(DEV)
        engines.append((eng, st, mass, n))
    for it in range(300):
        eng, st, mass, n = engines[it % 2]
        st[:, 7:10, :] *= (1.003 if it % 3 else 0.99)                  # new velocities -> every partial changes
        ke = eng.kinetic_energy(st, rotational=False)
        v = st[:, 7:10, :].permute(1, 0, 2).reshape(3, -1)[:, :n].double()
        want = (0.5 * mass * (v * v).sum(0)).sum().item()
        assert ke[0].item() == pytest.approx(want, rel=1e-12), it
    for eng, *_ in engines:
        eng.close()


def test_engine_holds_68_bytes_per_body_until_a_plain_soa_entry_is_used(native_built):
    """The engine's own buffers: tiled parameters (44 B) + tiled previous velocity (24 B) per body of capacity.  The
    plain-SoA copies (82 B more) appear with the first call of an entry point that takes plain field pointers."""
    cap = 1 << 22
    fx = load_golden("c2")
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    eng = HydroEngine(cap, DEV)
    eng.set_params(fx["params"][:4096], "f16")
    st = tiled(fx["state"]); pv = tiled(fx["prev"])
    w = eng.step_wrench_tiled(st, 4096, float(fx["dt"]), prev=pv)
    eng.step_wrench_tiled(st, 4096, float(fx["dt"]))                              # engine-owned previous velocity
    pos = torch.from_numpy(np.ascontiguousarray(fx["state"][:, 0:3])).to(DEV)
    quat = torch.from_numpy(np.ascontiguousarray(fx["state"][:, 3:7])).to(DEV)
    vel = torch.from_numpy(np.ascontiguousarray(fx["state"][:, 7:13])).to(DEV)
    eng.step_wrench_aos(pos, quat, vel, float(fx["dt"]), quat_xyzw=True)          # array-of-structs entry
    eng.kinetic_energy(st, rotational=True)
    eng.step_fused_tiled(st, tiled(np.zeros_like(fx["state"])), 4096, float(fx["dt"]))
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    per_body = (free0 - free1) / cap
    print(f"engine of {cap} bodies through the tiled / AoS / fused / KE entries: {per_body:.1f} B per body of capacity")
    assert per_body <= 80.0, per_body                                              # 68 + the test's own 4 096-body tensors
    out_plain = eng.step_wrench(soa(fx["state"]), float(fx["dt"]), prev=soa(fx["prev"]))     # first plain-SoA call: copies are made
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert 50.0 <= (free1 - free2) / cap <= 70.0, (free1 - free2) / cap            # 44 B parameters + 14 B fp16 coefficients
    assert np.array_equal(out_plain.cpu().numpy().T, scenes.from_tiled(w.cpu().numpy(), 4096))     # same bits through the lazy copy
    eng.set_params(fx["params"][:4096] * np.float32(1.0), "f32")                  # a later set_params refreshes the plain copy too
    a = eng.step_wrench(soa(fx["state"]), float(fx["dt"]), prev=soa(fx["prev"]))
    b = eng.step_wrench_tiled(st, 4096, float(fx["dt"]), prev=pv)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().T, scenes.from_tiled(b.cpu().numpy(), 4096))
    eng.close()


@pytest.mark.parametrize("order", ["params, reserve", "reserve, params", "reserve, params f16, params f32"])
def test_plain_soa_step_is_capturable_after_reserve_soa(order, native_built):
    """The first call of a plain-SoA entry allocates the engine's plain copies (not capturable); `reserve_soa` makes
    them up front, after which the entry is as capture-safe as the others: graph replay == eager call, bit for bit -
    in whichever order reserve_soa and set_params came (set_params keeps existing copies current: ADVICE r3)."""
    fx = load_golden("c2")
    n, dt = 4096, float(fx["dt"])
    eng = HydroEngine(n, DEV, float(fx["rho"]), float(fx["g"]))
    if order == "params, reserve":
        eng.set_params(fx["params"][:n])
        eng.reserve_soa()
    else:
        eng.reserve_soa()                                      # nothing to copy yet
        if "f16" in order:
            eng.set_params(fx["params"][:n] * np.float32(0.5), "f16")
        eng.set_params(fx["params"][:n])
    st, pv = soa(fx["state"][:n]), soa(fx["prev"][:n])
    out = torch.zeros((6, n), device=DEV)
    stream = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            eng.step_wrench(st, dt, out=out, prev=pv)          # the very first plain-SoA call of this engine, captured
        g.replay()
        stream.synchronize()
    eager = eng.step_wrench(st, dt, prev=pv)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    f, t = run_ext(fx["state"][:n], fx["prev"][:n], fx["params"][:n], float(fx["rho"]), float(fx["g"]), dt)
    assert np.array_equal(out.cpu().numpy().T, np.concatenate([f, t], axis=1))
    del g
    eng.close()


def test_integrator_and_closed_loop(native_built):
    # buoys (C2): the explicit toy integrator is only stable while damping * dt / mass < 2, which
    # the 0.45 kg SILVER2 links at 120 Hz violate (the reference leaves integration to PhysX)
    sc = scenes.scene_c2(n=1024)
    eng = HydroEngine(sc.n, DEV, sc.rho, sc.g)
    eng.set_params(sc.params)
    S = soa(sc.state)
    W = eng.step_wrench(S, sc.dt, prev=soa(sc.prev))
    S2 = eng.integrate(S, W, sc.dt)
    torch.cuda.synchronize()
    w6 = W.cpu().numpy().T
    ref = io.integrate(sc.state, w6, sc.params, sc.g, sc.dt)
    got = S2.cpu().numpy().T
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    # ... and per body and field group (tests/test_integrator_gpu.py has every entry)
    err = io.integrator_error_ulps(got, ref, sc.state, w6, sc.params, sc.g, sc.dt)
    assert io.max_error_ulps(err) <= io.STEP_ULP_BOUND, {g: float(e.max()) for g, e in err.items()}
    assert np.abs(np.linalg.norm(got[:, 3:7], axis=1) - 1).max() < 1e-6
    # closed loop, ping-pong state buffers: previous velocity = the other buffer's velocity rows
    A, B = S.clone(), torch.empty_like(S)
    prev = soa(sc.prev)
    for k in range(200):
        W = eng.step_wrench(A, sc.dt, out=W, prev=prev)
        eng.integrate(A, W, sc.dt, state_out=B)
        prev = A[7:13]                       # rows 7..12 of a (13,N) tensor are a contiguous (6,N) block
        A, B = B, A
    torch.cuda.synchronize()
    fin = A.cpu().numpy()
    assert np.isfinite(fin).all()
    assert np.abs(fin[7:10]).max() < 5.0     # damped, bounded: nothing exploded
    eng.close()


# ---------------- BASELINE full sizes: size-independent properties --------------------------
@pytest.fixture(scope="module")
def big_scene():
    base = scenes.scene_c5(n=131072, seed=55)
    reps = 8                                   # 1 048 576 bodies (config 5 size)
    rng = np.random.default_rng(0)
    idx = np.concatenate([rng.permutation(base.n) for _ in range(reps)])
    return scenes.Scene("C5", base.state[idx], base.prev[idx], base.params[idx], base.rho, base.g, base.dt, "f16"), base, idx


def test_full_size_properties(big_scene, native_built):
    sc, base, idx = big_scene
    assert sc.n == 1048576
    f, t = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt, "f16")
    assert np.isfinite(f).all() and np.isfinite(t).all()
    # (1) every copy of a body gets the same bits wherever it sits in the launch
    fb, tb = run_ext(base.state, base.prev, base.params, base.rho, base.g, base.dt, "f16")
    assert np.array_equal(f, fb[idx]) and np.array_equal(t, tb[idx])
    # (2) oracle on a strided subsample of the million
    sub = np.arange(0, sc.n, 257)
    rf, rt, aux = ho.step_wrench(sc.state[sub], sc.prev[sub], sc.params[sub], sc.rho, sc.g, sc.dt)
    err = ho.wrench_error(f[sub], t[sub], rf, rt, sc.params[sub], sc.rho, sc.g)
    assert err.max() <= GATE
    # (3) dry bodies: exact zeros
    ext = scenes.vertical_extent(sc.state[:, 3:7], sc.params[:, :3])
    dry = sc.state[:, 2].astype(np.float64) - ext > 0
    assert dry.sum() > 200000 and np.all(f[dry] == 0) and np.all(t[dry] == 0)
    # (4) the wrench does not depend on world x, y
    st = sc.state.copy(); st[:, 0] += 4321.0; st[:, 1] -= 999.5
    f2, t2 = run_ext(st, sc.prev, sc.params, sc.rho, sc.g, sc.dt, "f16")
    assert np.array_equal(f, f2) and np.array_equal(t, t2)
    # (5) clamp bound holds for every body
    assert np.all(np.linalg.norm(f.astype(np.float64), axis=1) <= sc.params[:, 10].astype(np.float64) * 500.0 * (1 + 1e-6))


def test_sharded_equals_unsharded_bit_for_bit(native_built):
    """Config 4 (262 144 bodies) cut into 8 contiguous shards of 32 768, as on 8 GPUs."""
    from silver2_isaacsim_amd.distributed import shard_range
    sc = scenes.scene_c4(n=262144, seed=4)
    f, t = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    ke_parts = []
    for r in range(8):
        lo, hi = shard_range(sc.n, r, 8)
        assert hi - lo == 32768
        sh = sc.shard(r, 8)
        fs, ts = run_ext(sh.state, sh.prev, sh.params, sh.rho, sh.g, sh.dt)
        assert np.array_equal(fs, f[lo:hi]) and np.array_equal(ts, t[lo:hi])
        eng = HydroEngine(sh.n, DEV, sh.rho, sh.g); eng.set_params(sh.params)
        ke_parts.append(eng.kinetic_energy(soa(sh.state)).cpu().numpy()[0]); eng.close()
    assert sum(ke_parts) == pytest.approx(ho.kinetic_energy(sc.state, sc.params)[0], rel=1e-12)


def test_yaw_equivariance_on_device(native_built):
    sc = scenes.scene_c4(n=65536, seed=12)
    th = 1.1
    c, s = np.cos(th), np.sin(th)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    st = sc.state.astype(np.float64).copy(); pv = sc.prev.astype(np.float64).copy()
    for a, b in ((0, 3), (7, 10), (10, 13)):
        st[:, a:b] = st[:, a:b] @ rz.T
    pv[:, 0:3] = pv[:, 0:3] @ rz.T; pv[:, 3:6] = pv[:, 3:6] @ rz.T
    x, y, z, w = (sc.state[:, 3 + i].astype(np.float64) for i in range(4))
    a, b, cc, d = 0.0, 0.0, np.sin(th / 2), np.cos(th / 2)
    st[:, 3] = d * x + a * w + b * z - cc * y; st[:, 4] = d * y - a * z + b * w + cc * x
    st[:, 5] = d * z + a * y - b * x + cc * w; st[:, 6] = d * w - a * x - b * y - cc * z
    f0, t0 = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    f1, t1 = run_ext(st.astype(np.float32), pv.astype(np.float32), sc.params, sc.rho, sc.g, sc.dt)
    # The rotated inputs are re-rounded to fp32 (6e-8 relative per input), so this is a conditioning statement, not a
    # rounding one: the kernel's own error is ~1e-7 (its fp64 body), what is left is the model's sensitivity to 6e-8
    # input perturbations.  The oracle sees the same thing on the same rounded inputs - compare with IT at the parity
    # gate, and report the equivariance residual itself.
    err = ho.wrench_error(f1, t1, f0.astype(np.float64) @ rz.T, t0.astype(np.float64) @ rz.T, sc.params, sc.rho, sc.g)
    rf, rt, _ = ho.step_wrench(st.astype(np.float32), pv.astype(np.float32), sc.params, sc.rho, sc.g, sc.dt)
    err_or = ho.wrench_error(f1, t1, rf, rt, sc.params, sc.rho, sc.g)
    print(f"[yaw] equivariance residual p50 {np.median(err):.2e} p99 {np.percentile(err, 99):.2e} max {err.max():.2e}; "
          f"vs the oracle on the rotated inputs: max {err_or.max():.2e}")
    assert err_or.max() <= 5e-7                       # kernel vs oracle on the SAME (rotated, re-rounded) inputs: the parity bound
    assert np.percentile(err, 99) < 2e-5 and np.median(err) < 5e-7     # what re-rounding the inputs costs (was 2e-4)


# ---------------- tiled struct-of-arrays: the engine's native layout -----------------------
def tiled(x):
    return torch.from_numpy(scenes.to_tiled(x)).to(DEV)


@pytest.mark.parametrize("name", ["c2", "c4", "c5"])
@pytest.mark.parametrize("n", [None, 1, 63, 64, 65, 1000])
def test_tiled_entry_same_bits_as_plain_soa(name, n, native_built):
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = n or len(fx["state"])
    coeff = "f16" if name == "c5" else "f32"
    st, pv, pr = fx["state"][:n], fx["prev"][:n], fx["params"][:n]
    f_ref, t_ref = run_ext(st, pv, pr, rho, g, dt, coeff)
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(pr, coeff)
    S = tiled(st)
    for block in (128, 256):
        for nt in (0, 1):
            eng.set_tuning(0, block, nt)
            out = eng.step_wrench_tiled(S, n, dt, prev=tiled(pv))
            torch.cuda.synchronize()
            o = scenes.from_tiled(out.cpu().numpy(), n)
            assert np.array_equal(o[:, :3], f_ref) and np.array_equal(o[:, 3:], t_ref), (block, nt)
    # the residency cap (a dynamic-LDS request, the kernel uses none) changes scheduling only
    for waves in (2, 4, 5, 8):
        eng.set_tuning(0, 0, -1, waves)
        o = scenes.from_tiled(eng.step_wrench_tiled(S, n, dt, prev=tiled(pv)).cpu().numpy(), n)
        assert np.array_equal(o[:, :3], f_ref) and np.array_equal(o[:, 3:], t_ref), waves
    # padding lanes of the last tile are never written
    eng.set_tuning(0, 0, -1)
    out = torch.full((eng.tiles(n), 6, 64), -5.0, device=DEV)
    eng.step_wrench_tiled(S, n, dt, out=out, prev=tiled(pv))
    flat = out.cpu().numpy().transpose(0, 2, 1).reshape(-1, 6)
    assert np.all(flat[n:] == -5.0)
    # oracle gate as well
    rf, rt, _ = ho.step_wrench(st, pv, pr, rho, g, dt)
    assert ho.wrench_error(flat[:n, :3], flat[:n, 3:], rf, rt, pr, rho, g).max() <= GATE
    eng.close()


@pytest.mark.parametrize("coeff", ["f32", "f16"])
@pytest.mark.parametrize("own_prev", [False, True])
def test_batched_scenes_in_one_launch_give_the_bits_of_single_launches(coeff, own_prev, native_built):
    """hydro_step_wrench_tiled_batch: k independent scenes, one launch.  Ragged sizes (1, 63, 257, 4096, 100 003 bodies:
    scenes that end inside a tile and inside a block), different scene scalars per scene, caller-owned or engine-owned
    previous velocity: every scene's wrench (and, engine-owned, its stored previous velocity) has the bits of its own
    hydro_step_wrench_tiled call."""
    sizes = [4096, 1, 257, 100003, 63, 1000]
    engines, states, prevs, refs, host_prev, first_prev = [], [], [], [], [], []
    for k, n in enumerate(sizes):
        sc = scenes.scene_c4(n=n, seed=100 + k)
        eng = HydroEngine(n, DEV, 1000.0 + 5.0 * k, 9.81 - 0.01 * k)               # scene scalars differ
        eng.set_params(sc.params, coeff)
        st, pv = tiled(sc.state), tiled(sc.prev)
        if own_prev:
            eng.set_prev_velocity(sc.prev)
            refs.append(eng.step_wrench_tiled(st, n, sc.dt).clone())
            eng.set_prev_velocity(sc.prev)
        else:
            refs.append(eng.step_wrench_tiled(st, n, sc.dt, prev=pv).clone())
        engines.append(eng); states.append(st); prevs.append(pv); host_prev.append(sc.state[:, 7:13]); first_prev.append(sc.prev)
    dt = scenes.scene_c4(n=1).dt
    outs = HydroEngine.step_wrench_tiled_batch(engines, states, dt, prevs=None if own_prev else prevs)
    torch.cuda.synchronize()
    for k, (o, r) in enumerate(zip(outs, refs)):
        assert torch.equal(o, r), f"scene {k} ({sizes[k]} bodies)"
        if own_prev:
            assert np.array_equal(engines[k].get_prev_velocity().cpu().numpy().T, host_prev[k])
    # a launch of at most four scenes takes the short kernarg table, a kernel instantiation of its own: same bits
    few = 3
    if own_prev:
        for k in range(few):
            engines[k].set_prev_velocity(first_prev[k])
    outs_few = HydroEngine.step_wrench_tiled_batch(engines[:few], states[:few], dt, prevs=None if own_prev else prevs[:few])
    torch.cuda.synchronize()
    for k in range(few):
        assert torch.equal(outs_few[k], refs[k]), f"short table, scene {k} ({sizes[k]} bodies)"
        if own_prev:
            assert np.array_equal(engines[k].get_prev_velocity().cpu().numpy().T, host_prev[k])
    # prepared form: re-issued, follows the buffers' contents; the previous STATE buffer's velocity fields serve as prev
    if not own_prev:
        prev_states = []
        for k, n in enumerate(sizes):
            ps = torch.zeros((HydroEngine.tiles(n), 13, 64), device=DEV); ps[:, 7:13, :] = prevs[k]
            prev_states.append(ps)
        step, outs2 = HydroEngine.prepare_step_wrench_tiled_batch(engines, states, dt, prevs=prev_states)
        step(); torch.cuda.synchronize()
        assert all(torch.equal(o, r) for o, r in zip(outs2, refs))
        states[3][:, 2, :] -= 0.125
        step(); torch.cuda.synchronize()
        assert torch.equal(outs2[3], engines[3].step_wrench_tiled(states[3], sizes[3], dt, prev=prevs[3])) and not torch.equal(outs2[3], refs[3])
    for e in engines:
        e.close()


def test_batched_launch_refuses_what_one_kernel_instance_cannot_serve(native_built):
    fx = load_golden("c2")
    n, dt = 512, float(fx["dt"])
    def make(coeff="f32", sem="numba"):
        e = HydroEngine(n, DEV); e.set_params(fx["params"][:n], coeff); e.set_semantics(sem); return e
    a, b = make(), make()
    st, pv = tiled(fx["state"][:n]), tiled(fx["prev"][:n])
    HydroEngine.step_wrench_tiled_batch([a, b], [st, st], dt, prevs=[pv, pv])            # fine
    with pytest.raises(HydroError, match="share"):                                         # f32 and f16 records in one launch
        c = make("f16"); HydroEngine.step_wrench_tiled_batch([a, c], [st, st], dt, prevs=[pv, pv])
    with pytest.raises(HydroError, match="once per launch"):                               # engine-owned prev, same engine twice
        HydroEngine.step_wrench_tiled_batch([a, a], [st, st], dt)
    with pytest.raises(ValueError):
        HydroEngine.step_wrench_tiled_batch([a] * 33, [st] * 33, dt, prevs=[pv] * 33)
    with pytest.raises(HydroError, match="HYDRO_E_ARG"):
        HydroEngine.step_wrench_tiled_batch([a, b], [st, st], 0.0, prevs=[pv, pv])
    empty = HydroEngine(n, DEV)                                                             # no parameters set
    with pytest.raises(HydroError, match="HYDRO_E_STATE"):
        HydroEngine.step_wrench_tiled_batch([a, empty], [st, st], dt, prevs=[pv, pv], ns=[n, n])
    with pytest.raises(HydroError, match="empty scene"):
        HydroEngine.step_wrench_tiled_batch([a, b], [st, st], dt, prevs=[pv, pv], ns=[n, 0])
    for e in (a, b, c, empty):
        e.close()


def test_tiled_previous_velocity_modes(native_built):
    fx = load_golden("c4")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = 3000
    st, pv, pr = fx["state"][:n], fx["prev"][:n], fx["params"][:n]
    f_ref, t_ref = run_ext(st, pv, pr, rho, g, dt)
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(pr)
    S = tiled(st)
    # (a) previous STATE buffer passed in place: its velocity fields are the previous velocity
    prev_state = np.zeros((n, 13), np.float32); prev_state[:, 7:13] = pv
    out = eng.step_wrench_tiled(S, n, dt, prev=tiled(prev_state))
    o = scenes.from_tiled(out.cpu().numpy(), n)
    assert np.array_equal(o[:, :3], f_ref) and np.array_equal(o[:, 3:], t_ref)
    # (b) engine-owned: set -> step -> the engine holds this step's velocity; visible through the SoA getter
    eng.set_prev_velocity(pv)
    out = eng.step_wrench_tiled(S, n, dt)
    o = scenes.from_tiled(out.cpu().numpy(), n)
    assert np.array_equal(o[:, :3], f_ref) and np.array_equal(o[:, 3:], t_ref)
    assert np.array_equal(eng.get_prev_velocity().cpu().numpy().T, st[:, 7:13])
    eng.reset_prev_velocity()
    out0 = scenes.from_tiled(eng.step_wrench_tiled(S, n, dt).cpu().numpy(), n)
    f0, t0 = run_ext(st, np.zeros_like(pv), pr, rho, g, dt)
    assert np.array_equal(out0[:, :3], f0) and np.array_equal(out0[:, 3:], t0)
    eng.close()


def test_tiled_edges_pack_unpack_repack(native_built):
    fx = load_golden("c4")
    n = 2500
    st = fx["state"][:n]
    eng = HydroEngine(n, DEV)
    eng.set_params(fx["params"][:n])
    pos = torch.from_numpy(np.ascontiguousarray(st[:, 0:3])).to(DEV)
    q_wxyz = torch.from_numpy(np.ascontiguousarray(st[:, [6, 3, 4, 5]])).to(DEV)
    q_xyzw = torch.from_numpy(np.ascontiguousarray(st[:, 3:7])).to(DEV)
    vel = torch.from_numpy(np.ascontiguousarray(st[:, 7:13])).to(DEV)
    T = eng.pack_state_aos(pos, q_wxyz, vel)
    assert np.array_equal(scenes.from_tiled(T.cpu().numpy(), n), st)
    T2 = eng.pack_state_aos(pos, q_xyzw, vel, quat_xyzw=True)
    assert torch.equal(T, T2)
    # repack both ways is exact
    S = soa(st)
    assert torch.equal(eng.to_tiled(S)[:, :, :], T)
    assert torch.equal(eng.from_tiled(T, n), S)
    # wrench: tiled -> (n,3) forces / torques
    W = eng.step_wrench_tiled(T, n, float(fx["dt"]), prev=tiled(fx["prev"][:n]))
    F, Tq = eng.unpack_wrench_aos(W, n)
    w = scenes.from_tiled(W.cpu().numpy(), n)
    assert np.array_equal(F.cpu().numpy(), w[:, :3]) and np.array_equal(Tq.cpu().numpy(), w[:, 3:])
    eng.close()


def test_tiled_closed_loop_equals_plain_soa_loop(native_built):
    """200 ping-pong steps (wrench + integrator) in both layouts give the same trajectory bits."""
    sc = scenes.scene_c2(n=1000)
    eng = HydroEngine(sc.n, DEV, sc.rho, sc.g)
    eng.set_params(sc.params)
    n = sc.n
    A, B = soa(sc.state), torch.empty((13, n), device=DEV)
    prev = soa(sc.prev)
    At, Bt = tiled(sc.state), eng.alloc_tiled(13, n)
    prev_t = tiled(sc.prev)
    W, Wt = torch.empty((6, n), device=DEV), eng.alloc_tiled(6, n)
    for k in range(200):
        eng.step_wrench(A, sc.dt, out=W, prev=prev)
        eng.integrate(A, W, sc.dt, state_out=B)
        prev = A[7:13]
        A, B = B, A
        eng.step_wrench_tiled(At, n, sc.dt, out=Wt, prev=prev_t)
        eng.integrate_tiled(At, Wt, n, sc.dt, state_out=Bt)
        prev_t = At                                   # previous STATE buffer, used in place
        At, Bt = Bt, At
    torch.cuda.synchronize()
    fin = A.cpu().numpy().T
    assert np.isfinite(fin).all() and np.abs(fin[:, 7:10]).max() < 5.0
    assert np.array_equal(scenes.from_tiled(At.cpu().numpy(), n), fin)
    eng.close()


def test_engine_owned_previous_velocity_is_coherent_across_entry_points(native_built):
    """Plain-SoA, tiled and array-of-structs entries share ONE previous-velocity state."""
    fx = load_golden("c4")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = 1500
    st, pr = fx["state"][:n], fx["params"][:n]
    rng = np.random.default_rng(3)
    states = [st.copy() for _ in range(4)]
    for k, s_ in enumerate(states):
        s_[:, 7:13] += rng.normal(0, 0.05, (n, 6)).astype(np.float32) * k
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(pr)
    prev = np.zeros((n, 6), np.float32)
    outs = []
    for k, s_ in enumerate(states):
        if k % 3 == 0:
            o = eng.step_wrench(soa(s_), dt).cpu().numpy().T
        elif k % 3 == 1:
            o = scenes.from_tiled(eng.step_wrench_tiled(tiled(s_), n, dt).cpu().numpy(), n)
        else:
            pos = torch.from_numpy(np.ascontiguousarray(s_[:, 0:3])).to(DEV)
            q = torch.from_numpy(np.ascontiguousarray(s_[:, 3:7])).to(DEV)
            vel = torch.from_numpy(np.ascontiguousarray(s_[:, 7:13])).to(DEV)
            F, T = eng.step_wrench_aos(pos, q, vel, dt, quat_xyzw=True)
            o = np.concatenate([F.cpu().numpy(), T.cpu().numpy()], axis=1)
        f_ref, t_ref = run_ext(s_, prev, pr, rho, g, dt)
        assert np.array_equal(o[:, :3], f_ref) and np.array_equal(o[:, 3:], t_ref), k
        prev = s_[:, 7:13].copy()
        assert np.array_equal(eng.get_prev_velocity().cpu().numpy().T, prev)
    eng.close()


@pytest.mark.parametrize("scale", [1.0 + 1e-5, 1.001, 1.02, 0.9])
def test_non_unit_quaternions_are_used_as_given(scale, native_built):
    """N7: the reference never normalises the quaternion.  The kernels' cancellation-free forms rest on
    exact identities in e = |q|^2 - 1, so parity must hold for any |q|, not just for fp32-rounded unit ones."""
    sc = scenes.scene_c4(n=32768, seed=21)
    st = sc.state.copy()
    st[:, 3:7] = (st[:, 3:7].astype(np.float64) * scale).astype(np.float32)
    ext = scenes.vertical_extent(st[:, 3:7], sc.params[:, :3]); ext0 = scenes.vertical_extent(sc.state[:, 3:7], sc.params[:, :3])
    st[:, 2] = (sc.state[:, 2].astype(np.float64) * ext / ext0).astype(np.float32)     # keep dry/partial/full classes
    keep = scenes.branch_margins(st, sc.params) > 1e-4
    f, t = run_ext(st, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    rf, rt, _ = ho.step_wrench(st, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    err = ho.wrench_error(f, t, rf, rt, sc.params, sc.rho, sc.g)[keep]
    assert np.percentile(err, 99.9) < 3e-6 and (err > GATE).sum() == 0


def _components_both_entries(state, accel32, params, rho, g, coeff="f32"):
    """(n,8,3) + ratio from hydro_step_components (plain SoA) and from hydro_step_components_aos: they must agree bit for bit."""
    n = len(state)
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(params, coeff)
    comps, ratio = eng.step_components(soa(state), soa(accel32))
    c1 = comps.cpu().numpy().T.reshape(n, 8, 3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)    # noqa: E731
    out = torch.empty((8, n, 3), dtype=torch.float32, device=DEV)
    r2 = torch.empty((n,), dtype=torch.float32, device=DEV)
    eng.step_components_aos(dev(state[:, 0:3]), dev(state[:, 3:7]), dev(state[:, 7:10]), dev(state[:, 10:13]),
                            dev(accel32[:, 0:3]), dev(accel32[:, 3:6]), out, r2)
    torch.cuda.synchronize()
    c2 = out.cpu().numpy().transpose(1, 0, 2)
    assert np.array_equal(c1, c2) and torch.equal(ratio, r2)
    eng.close()
    return c1, ratio.cpu().numpy()


def _every_wrench_entry(state, prev, params, rho, g, dt):
    """The net wrench from hydro_step_wrench_ext (1 and 2 bodies per lane), _tiled and _aos (both quaternion orders):
    one set of bits."""
    f, t = run_ext(state, prev, params, rho, g, dt)
    f2, t2 = run_ext(state, prev, params, rho, g, dt, vec=2)
    assert np.array_equal(f, f2) and np.array_equal(t, t2)
    n = len(state)
    eng = HydroEngine(n, DEV, rho, g)
    eng.set_params(params)
    o = scenes.from_tiled(eng.step_wrench_tiled(tiled(state), n, dt, prev=tiled(prev)).cpu().numpy(), n)
    assert np.array_equal(o[:, :3], f) and np.array_equal(o[:, 3:], t)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)    # noqa: E731
    for xyzw in (False, True):
        eng.set_prev_velocity(prev)
        q = state[:, 3:7] if xyzw else state[:, [6, 3, 4, 5]]
        F, T = eng.step_wrench_aos(dev(state[:, 0:3]), dev(q), dev(state[:, 7:13]), dt, quat_xyzw=xyzw)
        assert np.array_equal(F.cpu().numpy(), f) and np.array_equal(T.cpu().numpy(), t)
    eng.close()
    return f, t


def test_degenerate_inputs(native_built):
    """Zero dimensions / mass / speed, -0.0, clamp, 10 km offsets, and every surface tie of the model (top / bottom /
    centre / face centre at z = 0, zero alignments, |axis| = 0) under four orientations - through every wrench entry and
    both component entries (tests/edge_cases.py; the table a mean-of-wet-points CoB fails)."""
    import edge_cases as ec
    f, t = _every_wrench_entry(ec.STATE, ec.PREV, ec.PARAMS, ec.RHO, ec.G, ec.DT)
    comps, ratio = _components_both_entries(ec.STATE, ec.ACCEL32, ec.PARAMS, ec.RHO, ec.G)
    ec.check(f, t, None, comps, ratio)


def test_surface_ties_through_every_entry(native_built):
    """tests/golden/ties.npz - 4 096 quantised bodies with keypoints / face centres EXACTLY on the surface under cube
    rotations and non-unit quaternions, outputs by the reference itself: net wrench within the gate through
    hydro_step_wrench_ext, _tiled and _aos, and the calculator surface through hydro_step_components and _aos (forces to
    1e-6 of the body's largest term, centres to half an fp32 ulp, cob = position exactly when the top keypoint is on the
    surface: numba_hydrodynamics.py:87-88)."""
    from edge_cases import check_components
    fx = load_golden("ties")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    f, t = _every_wrench_entry(fx["state"], fx["prev"], fx["params"], rho, g, dt)
    err = ho.wrench_error(f, t, fx["net_force"], fx["net_torque"], fx["params"], rho, g)
    assert err.max() <= GATE, f"{err.max():.3e} ({(err > GATE).sum()} bodies)"
    assert abs(t[0, 0] - (-533.9520915)) < 1e-3                        # the body of VERDICT r3 (+94.5 before the fix)
    dry = fx["ratio"] == 0.0
    assert dry.sum() > 1000 and np.all(f[dry] == 0.0) and np.all(t[dry] == 0.0)
    acc32 = accel_of(fx).astype(np.float32)
    comps, ratio = _components_both_entries(fx["state"], acc32, fx["params"], rho, g)
    ref = ho.solve_components(fx["state"], acc32.astype(np.float64), fx["params"].astype(np.float64), rho, g)
    check_components(comps, ratio, ref)
    for k in (6, 7):                                                    # centres straight against the reference's numbers
        want = fx["components"][:, k, :]
        tol = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) * (1 + 1e-6) + 1e-12
        assert np.all(np.abs(comps[:, k, :] - want) <= tol)
    top_tie = (fx["kind"] == 1) & (fx["ratio"] == 1.0)
    assert top_tie.sum() > 400 and np.array_equal(comps[top_tie, 6, :], fx["state"][top_tie, 0:3])
    # fp16 coefficients (config 5's storage): the same bodies, coefficients rounded to half first
    p16 = fx["params"].copy(); p16[:, 3:10] = p16[:, 3:10].astype(np.float16).astype(np.float32)
    f16, t16 = run_ext(fx["state"], fx["prev"], fx["params"], rho, g, dt, coeff="f16")
    rf, rt, _ = ho.step_wrench(fx["state"], fx["prev"], p16, rho, g, dt)
    assert ho.wrench_error(f16, t16, rf, rt, p16, rho, g).max() <= GATE


def test_quantised_fuzz_on_device(native_built):
    """The 200 000-body quantised population of tests/test_numerics_host.py::test_quantised_fuzz_host (another seed) on the
    DEVICE, whose reciprocals and roots are the seeded forms: wrench within the gate, ratio, and the calculator surface
    (centres to half an fp32 ulp) - every exact tie of the model decided as the reference decides it."""
    import populations
    from edge_cases import check_components
    st, pv, pr, kind = populations.surface_ties(n=200000, seed=777)
    f, t = run_ext(st, pv, pr, populations.RHO, populations.G, populations.DT)
    rf, rt, aux = ho.step_wrench(st, pv, pr, populations.RHO, populations.G, populations.DT)
    err = ho.wrench_error(f, t, rf, rt, pr, populations.RHO, populations.G)
    assert err.max() <= GATE, f"{(err > GATE).sum()} bodies above the gate, max {err.max():.3e}"
    dry = aux["ratio"] == 0.0
    assert np.all(f[dry] == 0.0) and np.all(t[dry] == 0.0)
    acc32 = ((st[:, 7:13].astype(np.float64) - pv.astype(np.float64)) / populations.DT).astype(np.float32)
    comps, ratio = _components_both_entries(st, acc32, pr, populations.RHO, populations.G)
    ref = ho.solve_components(st, acc32.astype(np.float64), pr.astype(np.float64), populations.RHO, populations.G)
    check_components(comps, ratio, ref)


def test_engine_lifetime_does_not_leak(native_built):
    """on_play / on_stop cycles create and drop engines: device memory must come back."""
    fx = load_golden("c2")

    def cycle():
        eng = HydroEngine(1 << 20, DEV)                       # ~190 MB of engine-owned buffers each
        eng.set_params(fx["params"][:1024])
        eng.step_wrench(soa(fx["state"][:1024]), 1 / 60)
        eng.close()
    cycle()                                                    # one-time costs: code objects, allocator pools
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(30):
        cycle()
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 64 << 20, (free0, free1)
    # many small handles at once (one per prim in per-prim mode), independent results
    engines = [HydroEngine(1, DEV) for _ in range(64)]
    outs = []
    for k, e in enumerate(engines):
        e.set_params(fx["params"][k:k + 1])
        outs.append(e.step_wrench(soa(fx["state"][k:k + 1]), float(fx["dt"]), prev=soa(fx["prev"][k:k + 1])))
    torch.cuda.synchronize()
    f, t = run_ext(fx["state"][:64], fx["prev"][:64], fx["params"][:64], float(fx["rho"]), float(fx["g"]), float(fx["dt"]))
    got = torch.cat(outs, dim=1).cpu().numpy().T
    assert np.array_equal(got[:, :3], f) and np.array_equal(got[:, 3:], t)
    for e in engines:
        e.close()
    e.close()                                                  # double close is harmless


def test_config5_every_body_against_the_oracle(native_built):
    """Config 5 at its real size, 1 048 576 DISTINCT bodies, fp16-stored coefficients: every body is
    compared with the fp64 C oracle (OpenMP over the host cores).  Gate 1e-5 on EVERY body, no allowance - and the
    tighter bound the fp64 evaluation delivers: 5e-7."""
    from oracle import c_oracle
    sc = scenes.scene_c5()                                   # seed 5, branch-margin rule applied
    assert sc.n == 1048576
    f, t = run_ext(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt, "f16")
    rf, rt = c_oracle.wrench(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt, threads=min(64, c_oracle.max_threads()))
    err = ho.wrench_error(f, t, rf, rt, sc.params, sc.rho, sc.g)
    over = int((err > GATE).sum())
    print(f"config 5, {sc.n} bodies: max {err.max():.3e}  p99.99 {np.percentile(err, 99.99):.3e}  "
          f"median {np.median(err):.3e}  bodies above 1e-5: {over}")
    assert np.isfinite(f).all() and np.isfinite(t).all()
    assert np.percentile(err, 99.99) < 3e-6
    assert over == 0 and err.max() <= 5e-7


@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_host_pointer_tables_for_params_and_prev(coeff, native_built):
    """on_device = 0: hydro_set_params_* / hydro_set_prev_velocity / hydro_get_prev_velocity take HOST arrays
    (what a C or Kit host without device copies of its constants would pass) - same bits as the device path."""
    import ctypes
    from silver2_isaacsim_amd import _native as nat
    fx = load_golden("c5")
    n = 777
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    st, pv, pr = fx["state"][:n], fx["prev"][:n], fx["params"][:n]
    ref = HydroEngine(n, DEV, rho, g)
    ref.set_params(pr, coeff); ref.set_prev_velocity(pv)
    S = tiled(st)
    want = ref.step_wrench_tiled(S, n, dt).clone()                      # engine-owned previous velocity
    want_prev = ref.get_prev_velocity().cpu().numpy()
    eng = HydroEngine(n, DEV, rho, g)
    lib = eng._lib
    host_params = [np.ascontiguousarray(pr[:, f], np.float32) for f in range(nat.PARAM_FIELDS)]
    host_prev = [np.ascontiguousarray(pv[:, f], np.float32) for f in range(nat.PREV_FIELDS)]
    fn = lib.hydro_set_params_f16 if coeff == "f16" else lib.hydro_set_params_f32
    assert fn(eng._h, n, nat.pointer_table([a.ctypes.data for a in host_params]), 0) == 0
    assert lib.hydro_set_prev_velocity(eng._h, n, nat.pointer_table([a.ctypes.data for a in host_prev]), 0) == 0
    eng.n, eng.coeff_dtype = n, coeff
    got = eng.step_wrench_tiled(S, n, dt)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    back = [np.empty(n, np.float32) for _ in range(nat.PREV_FIELDS)]
    assert lib.hydro_get_prev_velocity(eng._h, n, nat.pointer_table([a.ctypes.data for a in back]), 0) == 0
    assert lib.hydro_sync(eng._h) == 0
    assert np.array_equal(np.stack(back), want_prev) and np.array_equal(np.stack(back).T, st[:, 7:13])
    ref.close(); eng.close()


def test_handles_are_independent_across_host_threads(native_built):
    """not thread-safe per handle, safe across handles.  Four host threads, each with its own engine,
    stream and buffers, step concurrently; every thread gets the bits of the single-threaded run."""
    import threading
    fx = load_golden("c4")
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    n = 4096
    st, pv, pr = fx["state"][:n], fx["prev"][:n], fx["params"][:n]
    f_ref, t_ref = run_ext(st, pv, pr, rho, g, dt)
    results, errors = {}, []

    def worker(k):
        try:
            stream = torch.cuda.Stream(DEV)
            eng = HydroEngine(n, DEV, rho, g)
            eng.set_params(pr)
            S, P = tiled(st), tiled(pv)
            out = eng.alloc_tiled(6, n)
            with torch.cuda.stream(stream):
                for _ in range(300):
                    eng.step_wrench_tiled(S, n, dt, out=out, prev=P, stream=stream)
            stream.synchronize()
            results[k] = scenes.from_tiled(out.cpu().numpy(), n)
            eng.close()
        except Exception as e:                     # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not errors, errors
    for k in range(4):
        assert np.array_equal(results[k][:, :3], f_ref) and np.array_equal(results[k][:, 3:], t_ref), k


def test_maximum_tiled_size_addresses_every_tile(native_built):
    """Maximum sizes: the tiled kernels address with 32-bit byte offsets, so a tiled buffer may hold just under 4 GiB.
    78 copies of a 1 048 576-body scene = 81 788 928 bodies = 1 277 952 state tiles = 4.25 GB (99 % of the limit):
    every copy must come out with the bits of the 1 048 576-body launch - first, middle and last - and one more copy
    (4.31 GB) must be refused with HYDRO_E_ARG before anything is launched."""
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip("needs ~30 GB of device memory")
    sc = scenes.scene_c5(n=1048576, seed=5)
    copies, n1 = 78, sc.n
    t1 = n1 // 64
    small = HydroEngine(n1, DEV, sc.rho, sc.g)
    small.set_params(sc.params, "f16")
    st1 = tiled(sc.state)
    pv1 = tiled(sc.prev)
    ref = small.step_wrench_tiled(st1, n1, sc.dt, prev=pv1).clone()
    small.close()
    st1[:, 7:13, :] = pv1                                    # previous velocity in the state buffer's own velocity fields ...
    cur = st1.clone(); cur[:, 7:13, :] = tiled(sc.state)[:, 7:13, :]
    # ... so the big run can take its previous velocity in place from a second state buffer
    n = copies * n1
    big = HydroEngine(n + n1, DEV, sc.rho, sc.g)
    params = torch.from_numpy(np.ascontiguousarray(sc.params.T)).to(DEV).repeat(1, copies + 1)      # (11, n + n1)
    big.set_params(params, "f16")
    del params
    state = cur.repeat(copies, 1, 1)
    prev_state = st1.repeat(copies, 1, 1)
    assert state.numel() * 4 < 1 << 32 and (state.numel() + t1 * 832) * 4 >= 1 << 32
    out = big.step_wrench_tiled(state, n, sc.dt, prev=prev_state)
    torch.cuda.synchronize()
    for k in (0, copies // 2, copies - 1):
        assert torch.equal(out[k * t1:(k + 1) * t1], ref), k
    del out
    # one more copy: 4.31 GB - refused on its size (the same buffers are passed: nothing is dereferenced)
    with pytest.raises(HydroError, match="4 GiB"):
        big._check(big._lib.hydro_step_wrench_tiled(big._h, n + n1, state.data_ptr(), 13 * 64, prev_state.data_ptr() + 7 * 64 * 4, 13 * 64,
                                                   float(sc.dt), ref.data_ptr(), 6 * 64, None))
    big.close()
