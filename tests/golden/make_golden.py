#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by EXECUTING THE REFERENCE.

Runs only in the build container (needs /root/reference); the fixtures it
writes are committed, the reference never travels.  Usage:

    python3 -B tests/golden/make_golden.py                  (--only-ties, --only-params, --only-fuzz: those fixtures alone)

How the reference is run: Numba is not installed here,
so a stub module `numba` whose `njit(...)` is the identity decorator is placed
in `sys.modules`; the reference's function bodies are plain NumPy and execute
in float64.  `fastmath=True` only licenses re-association (~1e-15).  Nothing is
written into /root/reference (`sys.dont_write_bytecode`).

The behaviour-level epilogue is executed too: `hydrodynamics_behavior.py` is
imported with empty import shells for the Kit-only packages it names at module
level (omni, carb, pxr, isaacsim, warp - attribute access returns a dummy,
nothing of Kit is emulated), an instance is made with `object.__new__` (no
`on_init`), given an in-memory body view, the reference's Numba calculator and
float64 torch tensors, and the reference's own `_apply_behavior(dt)`
(hydrodynamics_behavior.py:176-238: wxyz->xyzw, finite-difference acceleration,
lever-arm torques, sum, clamp) runs unchanged; what it hands to
`apply_forces_and_torques_at_pos` is stored as `net_force` / `net_torque`.

What each fixture holds: fp32-exact inputs (state, acceleration or previous
velocity + dt, params, rho, g), the reference's nine outputs per body
(`solve_hydrodynamics`, numba_hydrodynamics.py:256-314) and the net wrench of
the reference's `_apply_behavior`, all float64.

N1 completion: for a wet body with speed <= 1e-6 the reference's
`calculate_pressure_and_area` returns None and `solve_hydrodynamics` raises
(TypeError under plain Python).  For those bodies only, this script calls the
reference's own sub-functions in the reference's order with
`(center_of_pressure, area) = (center_of_buoyancy, 0.0)` substituted, and
records the body in the fixture's `rest_completed` mask.
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

REFERENCE_SCRIPTS = "/root/reference/src/scripts"


class _Anything:
    """Import shell value: any attribute, any call; as a decorator it returns the function unchanged."""

    def __call__(self, *a, **k):
        if len(a) == 1 and callable(a[0]) and not isinstance(a[0], _Anything) and not k:
            return a[0]
        return _Anything()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()

    def __iter__(self):
        return iter(())


class _ShellModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "BehaviorScript":                     # must be subclassable
            return type("BehaviorScript", (object,), {})
        return _Anything()


KIT_ONLY = ["carb", "omni", "omni.kit", "omni.kit.window", "omni.kit.window.property", "omni.physx", "omni.kit.scripting",
            "omni.isaac", "omni.isaac.core", "omni.isaac.core.prims", "omni.isaac.core.simulation_context", "warp",
            "isaacsim", "isaacsim.replicator", "isaacsim.replicator.behavior", "isaacsim.replicator.behavior.global_variables",
            "isaacsim.replicator.behavior.utils", "isaacsim.replicator.behavior.utils.behavior_utils", "pxr"]


def import_reference():
    stub = types.ModuleType("numba")

    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn

    stub.njit = njit
    sys.modules["numba"] = stub
    for name in KIT_ONLY:
        if getattr(sys.modules.get(name), "IS_WARP_STANDIN", False):      # make_golden_warp.py: `warp` is executable there
            continue
        shell = _ShellModule(name)
        shell.__path__ = []
        sys.modules[name] = shell
    sys.path.insert(0, REFERENCE_SCRIPTS)
    import physics.numba_hydrodynamics as ref_k                    # noqa: E402
    import physics.numba_hydrodynamics_wrapper as ref_w            # noqa: E402
    import physics.hydrodynamics_behavior as ref_b                 # noqa: E402
    return ref_k, ref_w, ref_b


REF_K, REF_W, REF_B = import_reference()
import torch  # noqa: E402


def reference_body(state, accel, params, rho, g):
    """Nine reference outputs for one body -> (array (8,3), ratio, rest_completed)."""
    p, q, v, w = state[0:3], state[3:7], state[7:10], state[10:13]
    a, al = accel[0:3], accel[3:6]
    dims = [float(x) for x in params[0:3]]
    cd_lin, cd_ang, damp_lin, damp_ang, lift_c, am_lin, am_ang = (float(x) for x in params[3:10])
    wrap = REF_W.NumbaHydrodynamicsWrapper(
        dims[0], dims[1], dims[2], cd_lin, cd_ang, damp_lin, damp_ang,
        float(rho), float(g), am_lin, am_ang, lift_c)
    try:
        out = wrap.calculate_hydrodynamic_forces(p, q, v, w, a, al)
        return np.stack([np.asarray(o, dtype=np.float64) for o in out[:8]]), float(out[8]), False
    except TypeError:
        pass
    # ---- N1 completion, reference sub-functions in the reference's order ----
    f64 = lambda x: np.asarray(x, dtype=np.float64)                # noqa: E731
    p, q, v, w, a, al = map(f64, (p, q, v, w, a, al))
    rot = REF_K.quaternion_to_matrix(q)
    world = (rot @ wrap._local_keypoints.T).T + p
    ratio, cob = REF_K.analyze_submersion_and_cob(world, p)
    assert ratio > 1e-9, "TypeError is only expected on the wet rest branch"
    buoy = np.array([0.0, 0.0, wrap.water_density * (ratio * wrap.total_volume) * wrap.gravity])
    speed = np.linalg.norm(v)
    assert not speed > 1e-6
    vel_dir = np.zeros(3)
    cop, area = cob, 0.0
    drag_f, drag_t = REF_K.calculate_hybrid_drag(
        speed, vel_dir, ratio, wrap.water_density, area, wrap.total_volume,
        wrap.linear_drag_coefficient, wrap.linear_damping, v,
        wrap.angular_drag_coefficient, wrap.angular_damping, w)
    lift_f = REF_K.calculate_lift(speed, vel_dir, rot, area, wrap.water_density,
                                  wrap.lift_coefficient, ratio)
    am_f, am_t = REF_K.calculate_added_mass(ratio, a, al, rot, wrap._added_mass_matrix)
    comps = np.stack([f64(x) for x in (buoy, drag_f, lift_f, drag_t, am_f, am_t, cob, cop)])
    return comps, float(ratio), True


class _View:
    """In-memory stand-in for RigidPrimView: hands out the tensors, records what is applied."""

    def __init__(self, p, q_wxyz, vel6):
        self.p, self.q, self.v = p, q_wxyz, vel6
        self.applied = None

    def get_world_poses(self, clone=False):
        return self.p, self.q

    def get_velocities(self, clone=False):
        return self.v

    def apply_forces_and_torques_at_pos(self, forces=None, torques=None, positions=None, is_global=True):
        self.applied = (forces.clone(), torques.clone())


class _Calculator:
    """The reference's Numba calculator behind the tensor interface the behavior expects
    (8 tensors of shape (1,3)); N1 completion as in `reference_body`."""

    def __init__(self, params, rho, g):
        self.params, self.rho, self.g = params, rho, g
        self.last = None

    def calculate_hydrodynamic_forces(self, p, q, v, w, a, al):
        state = np.concatenate([x[0].numpy() for x in (p, q, v, w)])
        accel = np.concatenate([a[0].numpy(), al[0].numpy()])
        comps, ratio, rest = reference_body(state, accel, self.params, self.rho, self.g)
        self.last = (comps, ratio, rest)
        return tuple(torch.from_numpy(comps[k].copy())[None, :] for k in range(8))


def reference_behavior_wrench(state, prev, params, rho, g, dt):
    """Net (force, torque) of ONE body exactly as the reference's `_apply_behavior` computes them,
    in float64 (hydrodynamics_behavior.py:176-238 executed unchanged)."""
    f64 = lambda x: torch.tensor(np.asarray(x, dtype=np.float64)[None, :])   # noqa: E731
    s = np.asarray(state, dtype=np.float64)
    obj = object.__new__(REF_B.HydrodynamicsBehavior)
    obj._device = "cpu"
    obj._rigid_prim_view = _View(f64(s[0:3]), f64(s[[6, 3, 4, 5]]), f64(s[7:13]))     # simulator order: wxyz
    obj._hydro_calculator = _Calculator(params, rho, g)
    obj._mass = torch.tensor(float(params[10]), dtype=torch.float64)
    obj._last_linear_velocity = f64(prev[0:3])
    obj._last_angular_velocity = f64(prev[3:6])
    obj._apply_behavior(float(dt))
    f, t = obj._rigid_prim_view.applied
    assert torch.equal(obj._last_linear_velocity, f64(s[7:10]))                      # :237-238
    return f[0].numpy(), t[0].numpy()


def reference_behavior_batch(state, prev, params, rho, g, dt):
    n = state.shape[0]
    net_f, net_t = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        net_f[i], net_t[i] = reference_behavior_wrench(state[i], prev[i], params[i], rho, g, dt)
    return net_f, net_t


def reference_batch(state, accel, params, rho, g):
    n = state.shape[0]
    comps = np.zeros((n, 8, 3))
    ratio = np.zeros(n)
    rest = np.zeros(n, dtype=bool)
    for i in range(n):
        comps[i], ratio[i], rest[i] = reference_body(state[i], accel[i], params[i], rho, g)
    return comps, ratio, rest


def accel_from_prev(scene):
    """fp64 finite difference on the fp32-exact inputs (A13), what the fused path sees."""
    return (scene.state[:, 7:13].astype(np.float64) - scene.prev.astype(np.float64)) / np.float64(scene.dt)


def save_scene_fixture(name, scene, idx):
    state, prev, params = scene.state[idx], scene.prev[idx], scene.params[idx]
    accel = accel_from_prev(scene)[idx]
    comps, ratio, rest = reference_batch(state, accel, params, scene.rho, scene.g)
    net_f, net_t = reference_behavior_batch(state, prev, params, scene.rho, scene.g, scene.dt)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, index=np.asarray(idx, dtype=np.int64), state=state, prev=prev,
                        params=params, rho=np.float64(scene.rho), g=np.float64(scene.g),
                        dt=np.float64(scene.dt), components=comps, ratio=ratio, rest_completed=rest,
                        net_force=net_f, net_torque=net_t, scene_n=np.int64(scene.n))
    print(f"{name}: {len(idx)} bodies of {scene.n}, rest-completed {int(rest.sum())}, "
          f"dry {int((ratio == 0).sum())}, full {int((ratio == 1).sum())} -> {os.path.getsize(path)} B")


def subsample(n, head, total):
    """First `head` bodies plus an even stride through the rest, `total` indices."""
    rest = np.linspace(head, n - 1, total - head).astype(np.int64)
    return np.unique(np.concatenate([np.arange(head, dtype=np.int64), rest]))


def known_answer_cases():
    """K1-K5 of SURVEY.md section 8c (inputs as listed there)."""
    std = (1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02)   # cd_lin cd_ang damp_lin damp_ang lift am_lin am_ang
    def norm(q):
        q = np.asarray(q, dtype=np.float64)
        return q / np.linalg.norm(q)
    cases = [
        # name, dims, coeffs, p, q, v, w, a, alpha, mass
        ("K1", (1, 1, 1), std, (0.1, 0.2, -0.2), norm((0.1, 0.2, 0.3, 0.9)), (0.3, -0.1, 0.5),
         (0.2, 0.1, -0.4), (1, 2, 3), (-1, 0.5, 0.25), 500.0),
        ("K2", (0.26, 0.26, 0.30), (1.2, 0.8, 300.0, 150.0, 0.5, 0.2, 0.1), (2.0, 10.7, -18.4415),
         norm((0.05, -0.1, 0.7, 0.7)), (0.12, 0.03, -0.02), (0, 0.05, 0.3), (0.4, -0.2, 0.1), (0, 1, -2), 18.0),
        ("K3", (0.06, 0.09, 0.06), (1.0, 0.1, 20.0, 2.0, 0.1, 0.0, 0.0), (1, -2, -19),
         norm((0.3, 0.1, -0.2, 0.9)), (0.05, 0.02, -0.01), (0.01, -0.02, 0.05), (0.5, 0.5, 0.5), (1, 1, 1), 0.8),
        ("K4", (1, 1, 3), std, (-7, 40, 0.596), norm((0.02, -0.03, 0, 1)), (3, 0.5, -4),
         (0.1, 0.2, 0), (60, 0, -80), (0, 0, 0), 1.0),
        ("K5", (1, 1, 1), std, (0, 0, 5), (0, 0, 0, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), 1.0),
    ]
    names, state, accel, params = [], [], [], []
    for name, dims, co, p, q, v, w, a, al, mass in cases:
        names.append(name)
        state.append(np.concatenate([p, q, v, w]).astype(np.float64))
        accel.append(np.concatenate([a, al]).astype(np.float64))
        params.append(np.concatenate([dims, co, [mass]]).astype(np.float64))
    return names, np.stack(state), np.stack(accel), np.stack(params)


def save_known_answers():
    names, state, accel, params = known_answer_cases()
    comps, ratio, rest = reference_batch(state, accel, params, 1025.0, 9.81)
    dt = 1.0 / 60.0
    prev = state[:, 7:13] - accel * dt               # so that (v - v_last)/dt reproduces the listed acceleration
    net_f, net_t = reference_behavior_batch(state, prev, params, 1025.0, 9.81, dt)
    path = os.path.join(HERE, "kat.npz")
    np.savez_compressed(path, names=np.array(names), state=state, accel=accel, params=params, prev=prev, dt=np.float64(dt),
                        rho=np.float64(1025.0), g=np.float64(9.81), components=comps, ratio=ratio,
                        net_force=net_f, net_torque=net_t)
    for n_, f_, t_ in zip(names, net_f, net_t):
        print(f"  {n_}: net_F {f_} net_T {t_}")
    for n_, r_ in zip(names, ratio):
        print(f"  {n_}: ratio {r_!r}")
    print(f"kat: {len(names)} cases -> {os.path.getsize(path)} B")


def save_c1_trajectory():
    """Config 1: single buoy, 10 000 steps.  Forces from the reference functions;
    epilogue (hydrodynamics_behavior.py:212-226 restated in fp64) and a semi-implicit
    Euler point-mass integrator standing in for PhysX are this repo's own."""
    from silver2_isaacsim_amd import scenes
    from oracle import hydro_oracle as ho
    sc = scenes.scene_c1()
    steps = int(sc.info["steps"])
    params = sc.params[0].astype(np.float64)
    mass = params[10]
    dt = np.float64(sc.dt)
    p = sc.state[0, 0:3].astype(np.float64)
    q = sc.state[0, 3:7].astype(np.float64)
    v = sc.state[0, 7:10].astype(np.float64)
    w = np.zeros(3)
    v_last = np.zeros(3); w_last = np.zeros(3)
    z_hist = np.zeros(steps); vz_hist = np.zeros(steps); fz_hist = np.zeros(steps)
    rest_steps = []
    for k in range(steps):
        st = np.concatenate([p, q, v, w])
        acc = np.concatenate([(v - v_last) / dt, (w - w_last) / dt])
        comps, ratio, rest = reference_body(st, acc, params, sc.rho, sc.g)
        if rest:
            rest_steps.append(k)
        net_f, _net_t, _ = ho.behavior_epilogue_one(p, list(comps), mass)
        v_last = v.copy(); w_last = w.copy()
        v = v + dt * (net_f / mass + np.array([0.0, 0.0, -sc.g]))
        p = p + dt * v
        z_hist[k], vz_hist[k], fz_hist[k] = p[2], v[2], net_f[2]
    path = os.path.join(HERE, "c1_trajectory.npz")
    np.savez_compressed(path, z=z_hist, vz=vz_hist, fz=fz_hist, rest_steps=np.array(rest_steps, dtype=np.int64),
                        dt=dt, mass=np.float64(mass), params=params, rho=np.float64(sc.rho), g=np.float64(sc.g))
    print(f"c1: {steps} steps, z in [{z_hist.min():.6f}, {z_hist.max():.6f}], final z {z_hist[-1]:.6f}, "
          f"rest branch fired {len(rest_steps)}x -> {os.path.getsize(path)} B")


def save_ties():
    """Exact surface ties (tests/populations.py surface_ties): quantised bodies whose top / bottom keypoint, centre or
    a face centre has z = 0 EXACTLY, under cube rotations (fp32 sqrt(1/2) quarter turns, (1/2,1/2,1/2,1/2) thirds) and
    non-unit quaternions - the inputs on which `pz < 0` (numba_hydrodynamics.py:80), `z_min >= 0` / `z_max <= 0`
    (:86-87), `alignment > 0` (:132) and `norm(axis) < 1e-6` (:210) are decided on exact numbers.  Plus the one body
    of VERDICT r3 (unit cube, p_z = -1/2, quarter turn about x) as row 0."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import populations
    state, prev, params, kind = populations.surface_ties()
    s = np.float32(np.sqrt(0.5))
    state[0] = [0, 0, -0.5, s, 0, 0, s, 0.3, -0.1, 0.5, 0.2, 0.1, -0.4]
    prev[0] = 0.0
    params[0] = [1, 1, 1, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, 500.0]
    rho, g, dt = populations.RHO, populations.G, populations.DT
    accel = (state[:, 7:13].astype(np.float64) - prev.astype(np.float64)) / np.float64(dt)
    comps, ratio, rest = reference_batch(state, accel, params, rho, g)
    net_f, net_t = reference_behavior_batch(state, prev, params, rho, g, dt)
    path = os.path.join(HERE, "ties.npz")
    np.savez_compressed(path, state=state, prev=prev, params=params, kind=kind.astype(np.int8), rho=np.float64(rho), g=np.float64(g),
                        dt=np.float64(dt), components=comps, ratio=ratio, rest_completed=rest, net_force=net_f, net_torque=net_t)
    print(f"ties: {len(state)} bodies, rest-completed {int(rest.sum())}, dry {int((ratio == 0).sum())}, full {int((ratio == 1).sum())}; "
          f"{populations.tie_census(state, params)} -> {os.path.getsize(path)} B")
    print(f"  row 0 (VERDICT r3 body): net_T {net_t[0]}  cob {comps[0, 6]}")


def save_edge_cases():
    """The degenerate-input table of tests/edge_cases.py (zero dimensions / mass / speed, -0.0, clamp, 10 km offsets, every
    surface tie under four orientations) through the reference itself: the edge-case tests then compare the kernels with
    what the REFERENCE returns for these inputs, not only with the oracle's restatement of it."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import edge_cases as ec
    with np.errstate(all="ignore"):
        comps, ratio, rest = reference_batch(ec.STATE, ec.ACCEL, ec.PARAMS, ec.RHO, ec.G)
        net_f, net_t = reference_behavior_batch(ec.STATE, ec.PREV, ec.PARAMS, ec.RHO, ec.G, ec.DT)
    assert np.isfinite(comps).all() and np.isfinite(net_f).all() and np.isfinite(net_t).all()
    path = os.path.join(HERE, "edge_cases.npz")
    np.savez_compressed(path, names=np.array(ec.NAMES), state=ec.STATE, prev=ec.PREV, params=ec.PARAMS, rho=np.float64(ec.RHO),
                        g=np.float64(ec.G), dt=np.float64(ec.DT), components=comps, ratio=ratio, rest_completed=rest,
                        net_force=net_f, net_torque=net_t)
    print(f"edge_cases: {len(ec.NAMES)} cases, rest-completed {int(rest.sum())}, dry {int((ratio == 0).sum())} -> {os.path.getsize(path)} B")


def save_parameter_cases():
    """The parameter-record table of tests/parameter_cases.py (one constant of dims / coefficients / mass negative, zero, NaN,
    +-Inf or at an edge of the half format, on a wet moving body and on the same body lifted dry) through the reference itself:
    nine outputs per row and the net wrench of `_apply_behavior`, non-finite where the reference leaves them so, and `raised`
    where it raises instead of answering (those rows hold NaN)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import parameter_cases as pc
    names, state, prev, params = pc.table()
    n = len(names)
    accel = (state[:, 7:13].astype(np.float64) - prev.astype(np.float64)) / np.float64(pc.DT)
    comps, ratio = np.full((n, 8, 3), np.nan), np.full(n, np.nan)
    net_f, net_t = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    rest, raised = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            try:
                comps[i], ratio[i], rest[i] = reference_body(state[i], accel[i], params[i], pc.RHO, pc.G)
                net_f[i], net_t[i] = reference_behavior_wrench(state[i], prev[i], params[i], pc.RHO, pc.G, pc.DT)
            except Exception as e:                                     # noqa: BLE001  (whatever the reference raises is recorded)
                raised[i] = True
                comps[i], ratio[i], net_f[i], net_t[i] = np.nan, np.nan, np.nan, np.nan
                print(f"  {names[i]}: the reference raises {type(e).__name__}: {e}")
    path = os.path.join(HERE, "parameter_cases.npz")
    np.savez_compressed(path, names=np.array(names), state=state, prev=prev, params=params, rho=np.float64(pc.RHO), g=np.float64(pc.G),
                        dt=np.float64(pc.DT), components=comps, ratio=ratio, rest_completed=rest, net_force=net_f, net_torque=net_t,
                        raised=raised)
    finite = np.isfinite(net_f).all(axis=1) & np.isfinite(net_t).all(axis=1)
    print(f"parameter_cases: {n} rows, {int(finite.sum())} with a finite net wrench, {int(raised.sum())} raised, "
          f"dry {int((ratio == 0).sum())} -> {os.path.getsize(path)} B")


FUZZ_SEEDS = (20251, 20252)        # tests/test_reference_fuzz.py
FUZZ_BODIES = 3000                 # the fewest that still hold every count the test asserts (> 1000 thin plates, > 500 dry / full)


def save_fuzz(seed, n=FUZZ_BODIES):
    """The reference's outputs on tests/tools/reference_fuzz.py's special-value population(n, seed)."""
    sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
    import reference_fuzz as rf
    pop = rf.population(n, seed)
    ref = rf.reference_outputs(pop, sys.modules[__name__])
    path = rf.fixture_path(seed)
    np.savez_compressed(path, n=np.int64(n), seed=np.int64(seed), population_sha256=np.array(rf.population_digest(*pop[:3])),
                        **ref)
    print(f"fuzz_{seed}: {n} bodies, rest-completed {int(ref['rest_completed'].sum())}, "
          f"tiny {len(ref['tiny_index'])} -> {os.path.getsize(path)} B")


def main():
    from silver2_isaacsim_amd import scenes
    if "--only-ties" in sys.argv:
        save_ties()
        return save_edge_cases()
    if "--only-params" in sys.argv:
        return save_parameter_cases()
    if "--only-fuzz" in sys.argv:
        for seed in FUZZ_SEEDS:
            save_fuzz(seed)
        return
    save_known_answers()
    save_ties()
    save_edge_cases()
    save_parameter_cases()
    sc = scenes.scene_c2()
    save_scene_fixture("c2", sc, np.arange(sc.n))
    sc = scenes.scene_c3()
    save_scene_fixture("c3", sc, subsample(sc.n, 38, 1024))
    sc = scenes.scene_c4()
    save_scene_fixture("c4", sc, subsample(sc.n, 2048, 4096))
    sc = scenes.scene_c5()
    save_scene_fixture("c5", sc, subsample(sc.n, 1024, 2048))
    sc = scenes.scene_c4(n=2048, seed=44, margin=None)
    sc.name = "C4-adversarial"
    save_scene_fixture("c4_adversarial", sc, np.arange(sc.n))
    save_c1_trajectory()
    for seed in FUZZ_SEEDS:
        save_fuzz(seed)


if __name__ == "__main__":
    main()
