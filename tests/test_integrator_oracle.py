"""CPU checks of the integrator oracle (oracle/integrator_oracle.py) and of its metric.

The GPU tests (tests/test_integrator_gpu.py) hold every integrating entry to integrator_error_ulps <= STEP_ULP_BOUND
against `integrate`.  This file shows that this bound separates a wrong step from a right one: each mutant below - the
step with one typical mistake - lands above 100x the bound on at least 1 % (and at least 20) of the bodies of the
designed population and of samples of configs 2, 3 and 5.  It also pins the oracle itself: k = 0 is the explicit form,
and the translational part replays the config-1 trajectory of tests/golden/c1_trajectory.npz."""
import numpy as np
import pytest

import populations
from conftest import load_golden
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes

EXPLICIT_MUTANTS = ("no_gyro", "gyro_sign", "rotation_swapped", "inertia_permuted", "body_omega_in_quaternion",
                    "old_velocity_position", "no_gravity")
IMPLICIT_MUTANTS = ("k_unscaled", "den_plus", "implicit_no_gravity", "angular_explicit")
# config 3's links are near-cubic (0.26 x 0.26 x 0.30 m and 0.06 x 0.09 x 0.06 m) and turn at ~0.3 rad/s against
# damping torques of up to 150 N m s: there the gyroscopic term is 1e-5 .. 1e-4 of the torque term it is added to, and
# leaving it out (or flipping its sign) moves the angular velocity by 100 - 600 fp32 ulps of the field - 10x the bound,
# not 100x.  The population and configs 2 and 5 carry the 100x claim for those two mutants.
GYRO_FACTOR_C3 = 10.0


def _sample(name):
    if name == "population":
        st, pv, pr = populations.integrator_population()
        return st, pv, pr, populations.RHO, populations.G, populations.DT
    sc = {"c2": lambda: scenes.scene_c2(n=4096), "c3": lambda: scenes.scene_c3(envs=256),
          "c5": lambda: scenes.scene_c5(n=20000)}[name]()
    return sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt


@pytest.fixture(scope="module", params=["population", "c2", "c3", "c5"])
def sample(request):
    st, pv, pr, rho, g, dt = _sample(request.param)
    f, t, comps = ho.step_wrench(st, pv, pr, rho, g, dt)
    wrench = np.concatenate([f, t], axis=1).astype(np.float32)          # what the device hands its integrator
    return request.param, st, pr, rho, g, dt, wrench, comps


def _worst(err):
    return np.max(np.stack([np.nan_to_num(e, nan=np.inf) for e in err.values()]), axis=0)


@pytest.mark.parametrize("mutant", EXPLICIT_MUTANTS + IMPLICIT_MUTANTS)
def test_every_mutant_is_far_above_the_bound(sample, mutant):
    name, st, pr, rho, g, dt, wrench, comps = sample
    implicit = mutant in IMPLICIT_MUTANTS
    k = io.drag_jacobian(st, pr, comps, rho) if implicit else None
    ref = io.integrate(st, wrench, pr, g, dt, *(k or (None, None)))
    if mutant == "k_unscaled":
        if np.all(comps["scale"] == 1.0):
            # configs 2 and 3 have no body on which the clamp acts: the unscaled k IS the scaled one there
            assert name in ("c2", "c3")
            return
        ku = io.drag_jacobian(st, pr, dict(comps, scale=np.ones(len(st))), rho)
        bad = io.integrate(st, wrench, pr, g, dt, *ku)
    else:
        bad = io._step(st, wrench, pr, g, dt, *(k or (None, None)), mutate=(mutant,))
    worst = _worst(io.integrator_error_ulps(bad, ref, st, wrench, pr, g, dt, k))
    factor = GYRO_FACTOR_C3 if (name == "c3" and mutant in ("no_gyro", "gyro_sign")) else 100.0
    hit = int((worst > factor * io.STEP_ULP_BOUND).sum())
    print(f"[{name} {mutant}] {hit}/{len(st)} bodies above {factor:g} x {io.STEP_ULP_BOUND:g}, median {np.median(worst):.3g}")
    assert hit >= max(20, 0.01 * len(st)), (name, mutant, hit)


@pytest.mark.parametrize("name", ["population", "c3"])
def test_zero_k_is_the_explicit_form(name):
    st, pv, pr, rho, g, dt = _sample(name)
    f, t, _ = ho.step_wrench(st, pv, pr, rho, g, dt)
    wrench = np.concatenate([f, t], axis=1)
    zero = np.zeros(len(st))
    a = io.integrate(st, wrench, pr, g, dt)
    b = io.integrate(st, wrench, pr, g, dt, zero, zero)
    err = io.integrator_error_ulps(b, a, st, wrench, pr, g, dt)
    # fp64 rounding, in units of fp32 ulps of the field: 2^-29 per operation
    assert io.max_error_ulps(err) < 1e-6, io.max_error_ulps(err)


def test_drag_jacobian_is_the_drag_of_the_wrench():
    """k_lin v and k_ang w are the drag force / torque the oracle puts in the wrench (before the clamp), and the
    f16 variant uses the coefficients the fp16 record holds."""
    st, pv, pr = populations.integrator_population(n=4000, seed=32)
    rho, g, dt = populations.RHO, populations.G, populations.DT
    acc = ho.finite_difference_accel(st, pv, dt)
    c = ho.solve_components(st, acc, pr, rho, g)
    kl, ka = io.drag_jacobian(st, pr, c, rho)
    s = st.astype(np.float64)
    scale_f = np.maximum(np.abs(c["drag_force"]).max(axis=1), 1e-300)
    scale_t = np.maximum(np.abs(c["drag_torque"]).max(axis=1), 1e-300)
    assert (np.abs(kl[:, None] * s[:, 7:10] - c["drag_force"]).max(axis=1) <= 1e-12 * scale_f).all()
    assert (np.abs(ka[:, None] * s[:, 10:13] - c["drag_torque"]).max(axis=1) <= 1e-12 * scale_t).all()
    assert (kl <= 0).all() and (ka <= 0).all() and (kl < 0).mean() > 0.5
    p16 = pr.astype(np.float64)
    p16[:, 3:10] = p16[:, 3:10].astype(np.float16).astype(np.float64)
    c16 = ho.solve_components(st, acc, p16, rho, g)
    k16 = io.drag_jacobian(st, pr, c16, rho, "f16")
    assert np.array_equal(k16[0], io.drag_jacobian(st, p16, c16, rho)[0])
    assert not np.array_equal(k16[0], io.drag_jacobian(st, pr, c16, rho)[0])


def test_population_covers_what_it_promises():
    st, pv, pr = populations.integrator_population()
    rho, g, dt = populations.RHO, populations.G, populations.DT
    f, t, c = ho.step_wrench(st, pv, pr, rho, g, dt)
    kl, ka = io.drag_jacobian(st, pr, c, rho)
    m, inertia = pr[:, 10].astype(np.float64), io.box_inertia(pr)
    d = pr[:, 0:3].astype(np.float64)
    qn = np.linalg.norm(st[:, 3:7].astype(np.float64), axis=1)
    wn = np.linalg.norm(st[:, 10:13].astype(np.float64), axis=1)
    assert (scenes.branch_margins(st, pr) >= 1e-4).all()
    assert (np.abs(qn - 1) > 5e-4).sum() >= 500                                       # non-unit quaternions
    assert (d.max(axis=1) / d.min(axis=1) > 5).sum() >= 1000                           # slabs / rods
    assert (inertia.max(axis=1) / inertia.min(axis=1) > 10).sum() >= 200
    assert (wn > 8).sum() >= 200
    ratio = c["ratio"]
    assert min((ratio == 0).sum(), ((ratio > 0) & (ratio < 1)).sum(), (ratio == 1).sum()) >= 3000
    assert (c["scale"] < 1).sum() >= 2000
    kdt = np.abs(kl) * dt / m
    assert (kdt == 0).sum() >= 1000 and ((kdt > 1) & (kdt < 100)).sum() >= 1000 and ((kdt > 20) & (kdt < 100)).sum() >= 100
    assert (np.abs(st[:, 10:13]).max(axis=1) == 0).sum() >= 200 and (np.abs(st[:, 7:10]).max(axis=1) == 0).sum() >= 200
    assert np.abs(st[:, 0:3]).max() > 5e3


def test_translational_part_replays_the_config1_trajectory():
    """tests/golden/c1_trajectory.npz: z, v_z and the net F_z of every step of the fp64 point-mass loop of
    make_golden.py::save_c1_trajectory.  Fed the stored F_z, `integrate` reproduces the stored z / v_z sequence."""
    fx = load_golden("c1_trajectory")
    sc = scenes.scene_c1()
    params = fx["params"][None, :]
    dt, g = float(fx["dt"]), float(fx["g"])
    s = sc.state.astype(np.float64)
    z, vz = np.empty(len(fx["z"])), np.empty(len(fx["z"]))
    wrench = np.zeros((1, 6))
    for k in range(len(fx["z"])):
        wrench[0, 2] = fx["fz"][k]
        s = io.integrate(s, wrench, params, g, dt)
        z[k], vz[k] = s[0, 2], s[0, 9]
    assert np.abs(z - fx["z"]).max() <= 1e-12 and np.abs(vz - fx["vz"]).max() <= 1e-12
    assert np.array_equal(s[0, 3:7], [0.0, 0.0, 0.0, 1.0]) and not s[0, 10:13].any()    # no torque: attitude untouched
