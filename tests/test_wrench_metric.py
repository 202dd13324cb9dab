"""CPU checks of the per-component wrench metric (hydro_oracle.wrench_error_ulps) and of its longdouble reference.

The kernels evaluate the wrench in fp64 and round each output to fp32 once, so every component of a
body the clamp does not touch is within 2^-24 of its own terms: WRENCH_ULP_BOUND = 1 + 2^-8 units of ULP * s_i.  The
1e-5 gate of SURVEY.md 8d measures the error in norms with a floor, and cannot see an fp32 step that slipped back into
the fp64 body: such a step moves results by 1-3 fp32 ulps, 100x below the gate.  This file shows that the new bound does
see it.  Each mutant below - the wrench with one typical fp32 mistake - exceeds the bound on at least 20 bodies of the
population named for it, while the 1e-5 gate passes GATE_BLIND mutants on every body of c4 and c5.  The separation
comes from the bound being exact for correct rounding, not from a wide margin: the mutants reach 1.5-4 units.

The same metric holds the host instantiation of hydro_body.h (tests/host_emul) over every population, both semantics.
"""
import ctypes
import os

import numpy as np
import pytest

import wrench_ulps as wu
from conftest import REPO, SCENE_FIXTURES, load_golden
from oracle import hydro_oracle as ho

f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
POPULATIONS = list(wu.FIXTURES) + list(wu.CONDITIONING) + ["stress"]

# mutant -> the population on which it is asserted to exceed the bound on >= 20 bodies (test_mutant_table prints all).
# Where a mutant changes nothing measurable on a population, the reason:
#   * inv_dt_f32 on the fixtures and the conditioning sets (0 - 8 bodies over, 44 on `ties`): 1/dt rounded to fp32 is off
#     by ~0.4 ULP, and it only scales the added-mass terms, a small part of those wrenches - the slip stays below an
#     ulp of the sum.  The conditioning sets have no acceleration at all (prev = v).  On the stress population
#     (accelerations to 1e4 m/s^2) added mass dominates: 27 415 of 64 908 bodies over, max 2.8.
#   * g_f32 on terminal_rise: its bodies are chosen so that drag cancels buoyancy along z; the 4e-8 of g moves F_z by
#     4e-8 of B, below an ulp of the (larger) sum of magnitudes - the other populations carry it.
#   * heights_f32 on c3, terminal_rise: fully submerged or dry bodies, whose ratio is exactly 1 or 0 whatever the heights.
#   * inv_speed_seed on the floaters: at rest to 1e-4 m/s, where drag and lift are below an ulp of the buoyancy.
MUTANTS = {"g_f32": "c4", "inv_dt_f32": "stress", "rotation_f32": "c4", "arms_f32": "c4", "heights_f32": "c4",
           "inv_speed_seed": "c4", "terms_f32_sum": "c4", "drag_arm_cob": "c4"}
# The mutants the 1e-5 gate passes on every body of c4 and c5 - the gap this metric closes (old-gate max on c4 / c5):
# g_f32 4.9e-7 / 2.6e-7, inv_dt_f32 5.7e-8 / 5.9e-8, heights_f32 1.1e-7 / 1.1e-7, inv_speed_seed 1.5e-6 / 8.9e-6,
# terms_f32_sum 5.8e-7 / 3.8e-7.  (rotation_f32 reaches 1.8e-5 on c4; the fp32 lever arms and the CoB drag arm fail the
# gate outright.)
GATE_BLIND = ("g_f32", "inv_dt_f32", "heights_f32", "inv_speed_seed", "terms_f32_sum")
# host instantiation, clamp-active bodies: the count of CLAMP_ULP_BOUND with libm's correctly rounded sqrt and
# division (half an ulp, ULP relative, instead of the hardware's 1 ulp = 2 ULP): 7.5 ULP in all
HOST_CLAMP_BOUND = 7.5 + 2.0 ** -8


def mutant_wrench(name, st, pv, pr, rho, g, dt):
    """The wrench with one fp32 mistake, evaluated otherwise in fp64 and rounded to fp32 as the device returns it."""
    if name == "g_f32":                                    # the pre-0.2.0 float scene scalars
        f, t, _ = ho.step_wrench(st, pv, pr, rho, float(np.float32(g)), dt)
        return f.astype(np.float32), t.astype(np.float32)
    mutate = (name,) if name in ho.MUTATIONS else ()
    s64 = np.asarray(st, np.float64)
    if name == "inv_dt_f32":                               # 1/dt formed in fp32
        acc = (s64[:, 7:13] - np.asarray(pv, np.float64)) * float(np.float32(1.0) / np.float32(dt))
    else:
        acc = ho.finite_difference_accel(st, pv, dt)
    c = ho.solve_components(st, acc, pr, rho, g, mutate=mutate)
    p = s64[:, 0:3]
    if name == "arms_f32":                                 # world-space centres and lever arms formed in fp32
        for k in ("center_of_buoyancy", "center_of_pressure"):
            c[k] = p + f32(f32(c[k]) - f32(p))
    if name == "drag_arm_cob":                             # drag (and lift) lever arm from the CoB instead of the CoP
        c["center_of_pressure"] = c["center_of_buoyancy"]
    if name == "terms_f32_sum":                            # each term rounded to fp32, then an fp32 sum
        forces = [c[k] for k in ("buoyancy_force", "drag_force", "lift_force", "added_mass_force")]
        torques = [np.cross(c["center_of_buoyancy"] - p, c["buoyancy_force"]),
                   np.cross(c["center_of_pressure"] - p, c["drag_force"]),
                   np.cross(c["center_of_pressure"] - p, c["lift_force"]), c["drag_torque"], c["added_mass_torque"]]
        f = sum(x.astype(np.float32) for x in forces)
        t = sum(x.astype(np.float32) for x in torques)
        _, _, scale = ho.behavior_epilogue(p, c, pr[:, 10])
        return f * scale.astype(np.float32)[:, None], t * scale.astype(np.float32)[:, None]
    f, t, _ = ho.behavior_epilogue(p, c, pr[:, 10])
    return f.astype(np.float32), t.astype(np.float32)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in POPULATIONS:
        st, pv, pr, rho, g, dt = wu.population(name)
        out[name] = wu.Reference(st, pv, pr, rho, g, dt)
    return out


def _over(f, t, ref):
    """bodies above WRENCH_ULP_BOUND (clamp-active ones above CLAMP_ULP_BOUND, flipped ones excluded), the max."""
    e = ho.wrench_error_ulps(f, t, ref.ld, ref.state[:, 0:3])
    w = np.maximum(e["force"], e["torque"])
    w[list(ref.flips)] = 0.0
    over = np.where(e["clamped"], w > ho.CLAMP_ULP_BOUND, w > ho.WRENCH_ULP_BOUND)
    return int(over.sum()), float(w.max())


def test_mutant_table(refs):
    """Prints, per mutant and population, the bodies above the bound and the largest value; and the old gate's max."""
    print(f"\n{'mutant':16s}" + "".join(f"{p[:13]:>24s}" for p in POPULATIONS))
    for m in MUTANTS:
        row = []
        for name, ref in refs.items():
            f, t = mutant_wrench(m, ref.state, ref.prev, ref.params, ref.rho, ref.g, ref.dt)
            k, mx = _over(f, t, ref)
            old = ho.wrench_error(f, t, ref.f64[0], ref.f64[1], ref.params, ref.rho, ref.g).max()
            row.append(f"{k:>5d}/{len(f):<6d} {mx:5.3g} {old:6.1e}")
        print(f"{m:16s}" + "".join(f"{r:>24s}" for r in row))


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_exceeds_the_bound(refs, mutant):
    name = MUTANTS[mutant]
    ref = refs[name]
    f, t = mutant_wrench(mutant, ref.state, ref.prev, ref.params, ref.rho, ref.g, ref.dt)
    k, mx = _over(f, t, ref)
    print(f"[{mutant} on {name}] {k}/{len(f)} bodies above the bound, max {mx:.3g}")
    assert k >= 20, (mutant, name, k, mx)


@pytest.mark.parametrize("mutant", GATE_BLIND)
def test_the_old_gate_misses_these_mutants(refs, mutant):
    for name in ("c4", "c5"):
        ref = refs[name]
        f, t = mutant_wrench(mutant, ref.state, ref.prev, ref.params, ref.rho, ref.g, ref.dt)
        assert ho.wrench_error(f, t, ref.f64[0], ref.f64[1], ref.params, ref.rho, ref.g).max() <= wu.GATE, (mutant, name)


def test_the_correct_step_is_inside_the_bound(refs):
    """The fp64 oracle itself, rounded to fp32: the metric's own zero point (1 + fp64 noise)."""
    for name, ref in refs.items():
        k, mx = _over(ref.f64[0].astype(np.float32), ref.f64[1].astype(np.float32), ref)
        assert k == 0, (name, k, mx)


@pytest.mark.parametrize("name", ["kat"] + SCENE_FIXTURES)
def test_longdouble_reference_is_the_fp64_one(name):
    """dtype=np.longdouble changes the precision and nothing else: 1e-12 of the scale of every output (the lift: 1e-11,
    sin(2 asin d) is ill-conditioned where |d| -> 1, and costs the fp64 evaluation up to 4.4e-12 of the lift on c5)."""
    fx = load_golden(name)
    args = (fx["state"], fx["prev"], fx["params"], float(fx["rho"]), float(fx["g"]), float(fx["dt"]))
    a = ho.step_wrench(*args)
    b = ho.step_wrench(*args, dtype=np.longdouble)
    assert b[0].dtype == np.longdouble and b[2]["buoyancy_force"].dtype == np.longdouble
    floor = 1.0 if name == "ties" else 1e-12               # as test_oracle_golden: exact zeros of `ties` vs 5e-15 N
    for k in ho.COMPONENT_FIELDS + ("ratio", "scale"):
        x, y = np.asarray(a[2][k], np.float64), np.asarray(b[2][k], np.float64)
        den = np.maximum(np.abs(y).max(axis=-1), floor) if y.ndim > 1 else np.maximum(np.abs(y), floor)
        dif = np.abs(x - y).max(axis=-1) if y.ndim > 1 else np.abs(x - y)
        assert (dif <= (1e-11 if k == "lift_force" else 1e-12) * den).all(), k
    p = fx["state"][:, 0:3].astype(np.float64)
    s_f, s_t = ho.wrench_scales(p, b[2])
    assert (np.abs(a[0] - b[0]) <= 1e-12 * (s_f + floor)).all()
    # the torque: both evaluations form world-space centres and subtract p again (as the reference does), which costs
    # the fp64 one ~1e-16 |p| of every lever arm (c4: up to 2e-11 of s_t) - held to 1e-12 of that term as well
    forces = sum(np.linalg.norm(np.asarray(b[2][k], np.float64), axis=1)
                 for k in ("buoyancy_force", "drag_force", "lift_force"))
    arm_noise = (np.linalg.norm(p, axis=1) * forces)[:, None]
    assert (np.abs(a[1] - b[1]) <= 1e-12 * (s_t + arm_noise + floor)).all()
    assert len(ho.branch_flips(a[2], b[2])) == wu.EXPECTED_FLIPS.get(name, 0)


def test_metric_units():
    """One unit is 2^-24 of the component's own terms; sub-FLT_MIN components are held absolutely; a zero term set only
    passes an exact zero."""
    fx = load_golden("c4")
    ref = ho.step_wrench(fx["state"][:64], fx["prev"][:64], fx["params"][:64], float(fx["rho"]), float(fx["g"]),
                         float(fx["dt"]), dtype=np.longdouble)
    p = fx["state"][:64, 0:3]
    s_f, s_t = ho.wrench_scales(p, ref[2])
    f = (ref[0] + 3 * ho.ULP * s_f).astype(np.float64)
    e = ho.wrench_error_ulps(f, ref[1], ref, p)
    wet = ref[2]["ratio"] > 0                                # a dry body has no terms: s = 0, nothing was added
    assert wet.sum() > 20 and np.allclose(e["force"][wet], 3.0, rtol=1e-9) and np.all(e["force"][~wet] == 0)
    assert np.all(e["torque"] == 0)
    z = {k: np.zeros_like(v) for k, v in ref[2].items()}
    z["scale"] = np.ones(64); z["clamp_factor"] = np.full(64, 2.0)
    zero = (np.zeros((64, 3)), np.zeros((64, 3)), z)
    assert np.all(ho.wrench_error_ulps(np.zeros((64, 3)), np.zeros((64, 3)), zero, p)["force"] == 0)
    assert np.all(ho.wrench_error_ulps(np.full((64, 3), 1e-39), np.zeros((64, 3)), zero, p)["force"] == 0)   # < FLT_MIN
    assert np.all(np.isinf(ho.wrench_error_ulps(np.full((64, 3), 1e-30), np.zeros((64, 3)), zero, p)["force"]))


# ------------------------------------------------------------------------------ the host instantiation of hydro_body.h
@pytest.fixture(scope="module")
def emul(native_built):
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "host_emul", "libemul.so"))
    fp = ctypes.POINTER(ctypes.c_float)

    def run(state, prev, params, rho, g, dt, warp=False):
        n = len(state)
        f = np.empty((n, 3), np.float32); t = np.empty((n, 3), np.float32); r = np.empty(n, np.float32)
        st, pv, pr = (np.ascontiguousarray(x, np.float32) for x in (state, prev, params))
        lib.emul_set_semantics(int(warp))
        try:
            assert lib.emul_wrench(ctypes.c_int64(n), st.ctypes.data_as(fp), pv.ctypes.data_as(fp), pr.ctypes.data_as(fp),
                                   ctypes.c_double(rho), ctypes.c_double(g), ctypes.c_double(dt),
                                   f.ctypes.data_as(fp), t.ctypes.data_as(fp), r.ctypes.data_as(fp)) == 0
        finally:
            lib.emul_set_semantics(0)
        return f, t
    return run


@pytest.mark.parametrize("semantics", ["numba", "warp"])
def test_host_instantiation_is_correctly_rounded(emul, refs, semantics):
    print()
    for name in POPULATIONS + ["c4_131072_ungated"]:
        if semantics == "numba" and name in refs:
            ref = refs[name]
        else:
            ref = wu.Reference(*wu.population(name), semantics=semantics)
        f, t = emul(ref.state, ref.prev, ref.params, ref.rho, ref.g, ref.dt, semantics == "warp")
        m, mc, nc, nf = wu.check(f"host {name} {semantics}", f, t, ref, HOST_CLAMP_BOUND, wu.EXPECTED_FLIPS.get(name, 0))
        print(f"[host {semantics}] {name:22s} n={len(f):6d}  max {m:.4f} (bound {ho.WRENCH_ULP_BOUND:.4f})  "
              f"clamp-active {nc:5d} max {mc:.3f} (bound {HOST_CLAMP_BOUND:.3f})  branch flips {nf}")
