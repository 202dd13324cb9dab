"""`semantics="warp"`: where the reference's Warp twin (warp_hydrodynamics.py:233-335, the calculator
hydrodynamics_behavior.py:155 instantiates) differs from the Numba path (the tie rule of the centre
of buoyancy), and what pins it.

PINNED on the reference's Warp source AS EXECUTED: tests/golden/make_golden_warp.py runs warp_hydrodynamics.py and
warp_hydrodynamics_wrapper.py (unchanged) under tests/tools/warp_standin.py - a stand-in for the Warp runtime that
evaluates in float64, models Warp's zero-initialised locals (N1, N4: bodies on which they matter carry the `hole` flag)
and binds `quat_rotate` to the matrix form - through the reference's own `_apply_behavior`, and commits the outputs as
tests/golden/warp_reference.npz.  The oracle's Warp branch, the host instantiation of csrc/hydro_body.h and the HIP
entries are held to that fixture here.  NOT pinned: NVIDIA's runtime and its fp32 rounding.  Warp's own `quat_rotate`
is R(q) v + 2 (|q|^2 - 1) v; the kernels keep R(q) v, and `test_rotation_definition_effect` measures what that is worth
(SURVEY.md N9).  The default (Numba) mode must not move."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import hydro_oracle as ho
import populations

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import reference_fuzz as rfz  # noqa: E402

GATE = 1e-5


def _quat_z(deg):
    h = np.deg2rad(deg) / 2.0
    return np.array([0.0, 0.0, np.sin(h), np.cos(h)])


def test_oracle_warp_added_mass_closed_form():
    """Isotropic linear added mass: Numba gives -m a for any attitude, Warp gives -m R R a
    (warp_hydrodynamics.py:216-230): a 90 degree yaw turns the horizontal part of a by 180 degrees."""
    params = np.array([1.0, 1.0, 1.0, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, 500.0])
    p, v, w = np.array([0.0, 0.0, -5.0]), np.array([0.1, 0.0, 0.0]), np.zeros(3)
    a, alpha = np.array([1.0, 2.0, 3.0]), np.array([0.5, -1.0, 0.25])
    m = 1025.0 * 1.0 * 0.05
    nb = ho.solve_components_one(p, _quat_z(90), v, w, a, alpha, params, 1025.0, 9.81)
    wp = ho.solve_components_one(p, _quat_z(90), v, w, a, alpha, params, 1025.0, 9.81, semantics="warp")
    assert np.allclose(nb[4], -m * a, rtol=1e-12)
    assert np.allclose(wp[4], -m * np.array([-1.0, -2.0, 3.0]), rtol=1e-12, atol=1e-12)
    # cube: the angular diagonal is isotropic too (2 rho V c), same rotation rule
    mt = 1025.0 * 1.0 * 2.0 * 0.02
    assert np.allclose(nb[5], -mt * alpha, rtol=1e-12)
    assert np.allclose(wp[5], -mt * np.array([-0.5, 1.0, 0.25]), rtol=1e-12, atol=1e-12)
    for k in (0, 1, 2, 3, 6, 7):                      # everything else is common to the two calculators
        assert np.array_equal(nb[k], wp[k])
    # identity and half-turn attitudes: R = R^T, the two calculators agree
    for deg in (0, 180):
        x = ho.solve_components_one(p, _quat_z(deg), v, w, a, alpha, params, 1025.0, 9.81)
        y = ho.solve_components_one(p, _quat_z(deg), v, w, a, alpha, params, 1025.0, 9.81, semantics="warp")
        assert np.allclose(x[4], y[4], atol=1e-12) and np.allclose(x[5], y[5], atol=1e-12)


def test_oracle_warp_dry_body_centres():
    """N6: a dry body reports cob = cop = position in Warp (zeros in Numba); forces are zero in both."""
    params = np.array([1.0, 1.0, 1.0, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, 500.0])
    p = np.array([3.0, -4.0, 5.0])
    args = (p, _quat_z(30), np.ones(3), np.ones(3), np.ones(3), np.ones(3), params, 1025.0, 9.81)
    nb = ho.solve_components_one(*args)
    wp = ho.solve_components_one(*args, semantics="warp")
    assert all(np.all(x == 0.0) for x in nb[:8]) and nb[8] == 0.0
    assert all(np.all(x == 0.0) for x in wp[:6]) and wp[8] == 0.0
    assert np.array_equal(wp[6], p) and np.array_equal(wp[7], p)


def test_oracle_warp_cob_when_the_top_keypoint_is_on_the_surface():
    """No keypoint above the surface, the top nine exactly on it (z = 0 is not wet): Numba returns cob = position
    ("fully in by bounds", numba_hydrodynamics.py:87-88); the Warp twin has no such return and averages the 18 wet
    points (warp_hydrodynamics.py:58-61): cob_z = p_z - 0.25 for a unit cube.  Scalar and vectorised oracle alike."""
    params = np.array([1.0, 1.0, 1.0, 1.2, 0.8, 300.0, 150.0, 1.0, 0.05, 0.02, 500.0])
    p = np.array([2.0, -1.0, -0.5])
    args = (p, np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), params, 1025.0, 9.81)
    nb = ho.solve_components_one(*args)
    wp = ho.solve_components_one(*args, semantics="warp")
    assert nb[8] == wp[8] == 1.0
    assert np.array_equal(nb[6], p) and np.array_equal(wp[6], [2.0, -1.0, -0.75])
    st = np.concatenate([p, args[1], np.zeros(6)])[None, :]
    for sem, cob in (("numba", p), ("warp", [2.0, -1.0, -0.75])):
        c = ho.solve_components(st, np.zeros((1, 6)), params[None, :], 1025.0, 9.81, semantics=sem)
        assert np.array_equal(c["center_of_buoyancy"][0], cob) and np.array_equal(c["center_of_pressure"][0], cob)
    # fully submerged with all 27 points wet: the mean IS the position, in both
    deep = ho.solve_components(st - np.eye(13)[2], np.zeros((1, 6)), params[None, :], 1025.0, 9.81, semantics="warp")
    assert np.array_equal(deep["center_of_buoyancy"][0], p - [0.0, 0.0, 1.0])


@pytest.mark.parametrize("name", ["ties"])
def test_host_arithmetic_warp_mode_on_exact_ties(name, emul):
    """The host instantiation and the Warp oracle agree on the quantised bodies, whose top keypoints sit exactly on the
    surface.  Before the oracle's Warp CoB followed warp_hydrodynamics.py:58-61 there, their torques differed by up to
    ~100 % (the CoB lever arm); tests/test_wrench_metric.py found it."""
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    f, t = emul(fx["state"], fx["prev"], fx["params"], rho, g, dt, warp=True)
    rf, rt, _ = ho.step_wrench(fx["state"], fx["prev"], fx["params"], rho, g, dt, semantics="warp")
    assert ho.wrench_error(f, t, rf, rt, fx["params"], rho, g).max() <= GATE


def test_oracle_warp_scalar_equals_vectorised():
    fx = load_golden("c4")
    st, pr = fx["state"].astype(np.float64), fx["params"].astype(np.float64)
    acc = (st[:, 7:13] - fx["prev"].astype(np.float64)) / float(fx["dt"])
    rho, g = float(fx["rho"]), float(fx["g"])
    vec = ho.solve_components(st, acc, pr, rho, g, semantics="warp")
    for i in range(0, len(st), 7):
        one = ho.solve_components_one(st[i, 0:3], st[i, 3:7], st[i, 7:10], st[i, 10:13], acc[i, :3], acc[i, 3:], pr[i], rho, g,
                                      semantics="warp")
        for k, name in enumerate(ho.COMPONENT_FIELDS):
            assert np.allclose(vec[name][i], one[k], rtol=1e-12, atol=1e-12), (i, name)
    # and the mode matters on this scene: added mass differs from the Numba result for tilted bodies
    nb = ho.solve_components(st, acc, pr, rho, g)
    wet = nb["ratio"] > 0
    assert np.abs(vec["added_mass_force"][wet] - nb["added_mass_force"][wet]).max() > 1e-3


@pytest.fixture(scope="module")
def emul(native_built):
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "host_emul", "libemul.so"))
    fp = ctypes.POINTER(ctypes.c_float)

    def run(state, prev, params, rho, g, dt, warp):
        st = np.ascontiguousarray(state, np.float32); pv = np.ascontiguousarray(prev, np.float32)
        pr = np.ascontiguousarray(params, np.float32)
        n = len(st)
        f = np.empty((n, 3), np.float32); t = np.empty((n, 3), np.float32); r = np.empty(n, np.float32)
        lib.emul_set_semantics(int(warp))
        try:
            rc = lib.emul_wrench(ctypes.c_int64(n), st.ctypes.data_as(fp), pv.ctypes.data_as(fp), pr.ctypes.data_as(fp),
                                 ctypes.c_double(rho), ctypes.c_double(g), ctypes.c_double(float(dt)),
                                 f.ctypes.data_as(fp), t.ctypes.data_as(fp), r.ctypes.data_as(fp))
        finally:
            lib.emul_set_semantics(0)
        assert rc == 0
        return f, t
    return run


@pytest.mark.parametrize("name", ["c2", "c4", "c5"])
def test_host_arithmetic_warp_mode(name, emul):
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    f, t = emul(fx["state"], fx["prev"], fx["params"], rho, g, dt, warp=True)
    rf, rt, _ = ho.step_wrench(fx["state"], fx["prev"], fx["params"], rho, g, dt, semantics="warp")
    assert ho.wrench_error(f, t, rf, rt, fx["params"], rho, g).max() <= GATE
    # the default mode is untouched by the switch having been used
    f0, t0 = emul(fx["state"], fx["prev"], fx["params"], rho, g, dt, warp=False)
    assert ho.wrench_error(f0, t0, fx["net_force"], fx["net_torque"], fx["params"], rho, g).max() <= GATE


# ------------------------------------------------- the reference's Warp source as executed (warp_reference.npz)
WARP_POPULATIONS = ("c4", "c2", "ties", "edge", "fuzz")
BRANCH = {name: 1 << bit for bit, name in enumerate(ho.BRANCH_NAMES)}


class _WarpReference:
    """One population of tests/golden/warp_reference.npz with its inputs and the oracle's Warp branch on them, computed
    once per module and not changed by any test."""

    def __init__(self, name, pop, fx):
        self.name = name
        self.state, self.prev, self.params, self.rho, self.g, self.dt = pop
        for k in ("components", "net_force", "net_torque", "net_force_warp", "net_torque_warp", "finite", "hole", "unit",
                  "margin_ok", "formula_effect"):
            setattr(self, k, fx[f"{name}_{k}"])
        self.sha256 = str(fx[f"{name}_sha256"])
        self.accel = (self.state[:, 7:13].astype(np.float64) - self.prev.astype(np.float64)) / self.dt
        with np.errstate(all="ignore"):
            self.oracle = ho.solve_components(self.state, self.accel, self.params.astype(np.float64), self.rho, self.g, semantics="warp")
            self.oracle_numba = ho.solve_components(self.state, self.accel, self.params.astype(np.float64), self.rho, self.g)
            self.oracle_f, self.oracle_t, _ = ho.step_wrench(self.state, self.prev, self.params, self.rho, self.g, self.dt, semantics="warp")
        self.ok = self.finite & ~self.hole
        self.tiny = self.params[:, :3].min(axis=1) < rfz.TINY_DIMENSION
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def components_error(self, comps):
        """reference_fuzz.run's criterion: the largest difference of the eight outputs, forces and torques relative to
        max(1, the body's largest force / torque component), centres to max(1, the centre's largest coordinate)."""
        ref = self.components
        scale = np.maximum(1.0, np.abs(ref[:, :6]).max(axis=(1, 2)))
        with np.errstate(all="ignore"):
            return np.max([np.abs(comps[f] - ref[:, k]).max(axis=1) / (scale if k < 6 else np.maximum(1.0, np.abs(ref[:, k]).max(axis=1)))
                           for k, f in enumerate(ho.COMPONENT_FIELDS)], axis=0)

    def wrench_error(self, f, t, sel=slice(None)):
        """SURVEY 8d's metric against the fixture's net wrench (zero-volume bodies as reference_fuzz.run treats them)."""
        return rfz._wrench_error(ho, f, t, self.net_force[sel], self.net_torque[sel], self.params[sel], self.rho, self.g)


@pytest.fixture(scope="module")
def warp_reference():
    fx = load_golden("warp_reference")
    return {name: _WarpReference(name, pop, fx) for name, pop in populations.warp_reference_populations().items()}


def test_warp_reference_fixture_is_of_these_populations(warp_reference):
    assert tuple(warp_reference) == WARP_POPULATIONS
    sizes = {"c4": 1024, "c2": 512, "ties": 2048, "edge": 81, "fuzz": populations.WARP_FUZZ[0]}
    for name, r in warp_reference.items():
        assert len(r.state) == sizes[name] == len(r.components) == len(r.hole), name
        assert r.sha256 == rfz.population_digest(r.state, r.prev, r.params), \
            f"warp_reference.npz [{name}] was made from another population: python3 -B tests/golden/make_golden_warp.py"
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "warp_reference.npz")) <= 1 << 20


@pytest.mark.parametrize("name", WARP_POPULATIONS)
def test_oracle_warp_branch_against_the_executed_warp_source(warp_reference, name):
    """Every finite & ~hole body - exact ties, non-unit quaternions, zero dimensions included: the eight outputs within
    1e-9 of the body's scale, the net wrench of the reference's `_apply_behavior` within 1e-9 in the 8d metric."""
    r = warp_reference[name]
    d = r.components_error(r.oracle)
    e = r.wrench_error(r.oracle_f, r.oracle_t)
    print(f"[{name}] {int(r.ok.sum())} of {len(r.ok)} bodies: components max {np.nanmax(np.where(r.ok, d, 0)):.3e}, "
          f"net wrench max {np.nanmax(np.where(r.ok, e, 0)):.3e}")
    assert r.ok.sum() >= 0.75 * len(r.ok)
    bad = np.where(r.ok & ~(d <= 1e-9))[0]
    assert len(bad) == 0, (name, bad[:5], d[bad[:5]], r.state[bad[:1]], r.params[bad[:1]])
    bad = np.where(r.ok & ~(e <= 1e-9))[0]
    assert len(bad) == 0, (name, bad[:5], e[bad[:5]])


HOLE_CAP = {"c4": 0.02, "c2": 0.02, "fuzz": 0.02, "ties": 0.25, "edge": 0.25}


@pytest.mark.parametrize("name", WARP_POPULATIONS)
def test_warp_holes_are_few_and_completed_as_documented(warp_reference, name):
    """`hole`: a zero-initialised local of Warp's generated code mattered (N1: the function that falls off its end at
    speed <= 1e-6; N4: the unassigned lift direction).  Those bodies are left out of the comparisons above, so there may
    not be many - caps, not measurements.  Counted when the fixture was made: c4 8 of 1 024, c2 0 of 512, fuzz 11 of
    2 048, ties 496 of 2 048 (a quarter of them at rest and a quarter moving along an axis, by design), edge cases 20 of
    81.  On them the project's documented completion holds in the oracle: at rest the centre of pressure is the centre of
    buoyancy and the projected area 0 (N1); the lift is 0 (N1, N4).  And the flag covers the set the oracle predicts - a
    wet body whose lift has no direction, which includes every body at rest - and is exactly that set away from branches."""
    r = warp_reference[name]
    print(f"[{name}] hole on {int(r.hole.sum())} of {len(r.hole)} bodies")
    assert r.hole.sum() <= HOLE_CAP[name] * len(r.hole)
    o = r.oracle
    rest = r.hole & o["rest"]
    assert np.array_equal(o["center_of_pressure"][rest], o["center_of_buoyancy"][rest]) and np.all(o["area"][rest] == 0.0)
    assert np.all(o["lift_force"][r.hole] == 0.0)
    live, lift_ok = (o["branches"] & BRANCH["live"]) != 0, (o["branches"] & BRANCH["lift_ok"]) != 0
    predicted = live & ~lift_ok
    assert np.all(r.hole[predicted])
    away = r.unit & r.margin_ok                     # near a branch the run with Warp's own quat_rotate may decide otherwise
    assert np.array_equal(r.hole[away], predicted[away]), np.where(away & (r.hole != predicted))[0][:8]
    if name in ("ties", "edge", "fuzz"):
        assert rest.sum() > 0 and (r.hole & ~o["rest"]).sum() > 0          # both holes are met


def _axis_quaternion(state):
    q = state[:, 3:7]
    return ((np.abs(q) == 1.0).sum(axis=1) == 1) & ((q == 0.0).sum(axis=1) == 3)


def test_rotation_definition_effect(warp_reference):
    """Warp's `quat_rotate(q, v)` is v (2 w^2 - 1) + 2 w (u x v) + 2 u (u . v) = R(q) v + 2 (|q|^2 - 1) v; the Numba path
    and the kernels use R(q) v.  `formula_effect` is the 8d metric between the net wrenches of the two
    runs of the stand-in (never of the kernels).  Measured over unit & margin_ok & finite & ~hole: c4 1.000e-05 (1 016
    bodies: fp32-rounded unit quaternions, | |q|^2 - 1 | ~ 1e-7, amplified by the torque's cancellation), c2 1.430e-06
    (512 bodies).  Bounds by the project's rule, the next power of two at or above twice the measured value:
    c4 2^-15 = 3.05e-5, c2 2^-18 = 3.81e-6.  So a drop-in user who compares Warp mode with the Warp twin itself can see
    up to ~1e-5 on unit quaternions - the size of the gate - and differences of order one on non-unit ones.  Exactly 0
    where the quaternion is a signed basis vector: both definitions are exact there."""
    bound = {"c4": 2.0 ** -15, "c2": 2.0 ** -18}
    for name in ("c4", "c2"):
        r = warp_reference[name]
        sel = r.unit & r.margin_ok & r.ok
        worst = float(r.formula_effect[sel].max())
        print(f"[{name}] formula_effect max {worst:.3e} over {int(sel.sum())} bodies (bound {bound[name]:.3e})")
        assert sel.sum() >= 0.95 * len(sel)
        assert bound[name] / 4.0 < worst <= bound[name]
    exact = 0
    for name, r in warp_reference.items():
        sel = _axis_quaternion(r.state) & r.margin_ok & r.ok
        exact += int(sel.sum())
        assert np.all(r.formula_effect[sel & (r.params[:, :3].min(axis=1) > 0)] == 0.0), name     # (zero volume: the metric is 0 / 0)
        assert np.array_equal(r.net_force[sel], r.net_force_warp[sel]) and np.array_equal(r.net_torque[sel], r.net_torque_warp[sel])
    assert exact >= 20
    fz = warp_reference["fuzz"]                       # non-unit quaternions, used as given: the two definitions part
    assert np.nanmax(fz.formula_effect[fz.ok & ~fz.unit & ~fz.tiny]) > 0.1


def _mutant(r, which):
    """The oracle's Warp outputs with ONE of the things that make it Warp undone (taken from its Numba branch)."""
    o, nb = dict(r.oracle), r.oracle_numba
    live = (o["branches"] & BRANCH["live"]) != 0
    if which == "added mass rotated with R^T":
        o["added_mass_force"], o["added_mass_torque"] = nb["added_mass_force"], nb["added_mass_torque"]
    elif which == "fully-in centre of buoyancy = position on ties":
        for k in ("center_of_buoyancy", "center_of_pressure"):
            o[k] = np.where(live[:, None], nb[k], o[k])
    elif which == "dry centres zero":
        for k in ("center_of_buoyancy", "center_of_pressure"):
            o[k] = np.where(live[:, None], o[k], 0.0)
    else:
        raise ValueError(which)
    return o


@pytest.mark.parametrize("which", ["added mass rotated with R^T", "fully-in centre of buoyancy = position on ties",
                                   "dry centres zero"])
def test_fixture_catches_each_warp_mutant(warp_reference, which):
    """The 1e-9 comparison separates the Warp branch from a branch with one typical mistake: each mutant is off the
    fixture by more than 1e-3 of the body's scale - a million times the bound - on at least 20 bodies of a population."""
    hits = {}
    for name, r in warp_reference.items():
        d = r.components_error(_mutant(r, which))
        hits[name] = int((r.ok & (d > 1e-3)).sum())
    print(f"[{which}] bodies off by more than 1e-3: {hits}")
    assert max(hits.values()) >= 20, hits
    assert all(int((r.ok & ~(r.components_error(r.oracle) <= 1e-9)).sum()) == 0 for r in warp_reference.values())


@pytest.fixture(scope="module")
def emul_components(native_built):
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "host_emul", "libemul.so"))
    fp = ctypes.POINTER(ctypes.c_float)

    def run(state, accel, params, rho, g, warp):
        st = np.ascontiguousarray(state, np.float32); ac = np.ascontiguousarray(accel, np.float32)
        pr = np.ascontiguousarray(params, np.float32)
        n = len(st)
        out = np.empty((n, 8, 3), np.float32); ratio = np.empty(n, np.float32)
        lib.emul_set_semantics(int(warp))
        try:
            rc = lib.emul_components(ctypes.c_int64(n), st.ctypes.data_as(fp), ac.ctypes.data_as(fp), pr.ctypes.data_as(fp),
                                     ctypes.c_double(rho), ctypes.c_double(g), out.ctypes.data_as(fp), ratio.ctypes.data_as(fp))
        finally:
            lib.emul_set_semantics(0)
        assert rc == 0
        return out
    return run


def _centre_tolerance(want):
    """reference_fuzz.run's: half an fp32 ulp of the coordinate + 1e-6."""
    return 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) * (1 + 1e-6) + 1e-6


@pytest.mark.parametrize("name", WARP_POPULATIONS)
def test_host_arithmetic_warp_mode_against_the_executed_warp_source(warp_reference, name, emul, emul_components):
    """The host instantiation of csrc/hydro_body.h in Warp mode on finite & ~hole bodies that are not tiny
    (reference_fuzz.TINY_DIMENSION): net wrench inside the 1e-5 gate; centres within half an fp32 ulp + 1e-6; buoyancy,
    drag force, lift and drag torque within 1e-6 of the body's largest term (reference_fuzz.run's tolerances)."""
    r = warp_reference[name]
    sel = r.ok & ~r.tiny
    with np.errstate(all="ignore"):
        f, t = emul(r.state, r.prev, r.params, r.rho, r.g, r.dt, warp=True)
        err = r.wrench_error(f, t)
    print(f"[{name}] {int(sel.sum())} bodies: net wrench max {np.nanmax(np.where(sel, err, 0)):.3e}")
    bad = np.where(sel & ~(err <= GATE))[0]
    assert len(bad) == 0, (name, bad[:5], err[bad[:5]])
    out = emul_components(r.state, r.accel, r.params, r.rho, r.g, warp=True)
    for k in (6, 7):
        want = r.components[:, k]
        bad = np.where(sel & (np.abs(out[:, k] - want) > _centre_tolerance(want)).any(axis=1))[0]
        assert len(bad) == 0, (name, ho.COMPONENT_FIELDS[k], bad[:5], out[bad[:2], k], want[bad[:2]])
    scale = np.maximum(1.0, np.abs(r.components[:, :6]).max(axis=(1, 2)))
    for k in (0, 1, 2, 3):
        bad = np.where(sel & (np.abs(out[:, k] - r.components[:, k]).max(axis=1) > 1e-6 * scale))[0]
        assert len(bad) == 0, (name, ho.COMPONENT_FIELDS[k], bad[:5])


# ------------------------------------------------------------------------------------------- GPU
def _engine(n, rho, g, params, coeff="f32", semantics="numba"):
    from silver2_isaacsim_amd.engine import HydroEngine
    eng = HydroEngine(n, "cuda:0", rho, g)
    eng.set_params(params, coeff)
    eng.set_semantics(semantics)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "c4", "c5"])
def test_gpu_wrench_warp_mode_every_entry(name, native_built):
    import torch
    from silver2_isaacsim_amd import scenes
    fx = load_golden(name)
    rho, g, dt = float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    st, pv, pr = fx["state"], fx["prev"], fx["params"]
    n = len(st)
    rf, rt, _ = ho.step_wrench(st, pv, pr, rho, g, dt, semantics="warp")
    eng = _engine(n, rho, g, pr, "f16" if name == "c5" else "f32", "warp")
    dev = "cuda:0"
    soa = eng.step_wrench(torch.from_numpy(scenes.to_soa(st)).to(dev), dt, prev=torch.from_numpy(scenes.to_soa(pv)).to(dev)).cpu().numpy().T
    til = scenes.from_tiled(eng.step_wrench_tiled(torch.from_numpy(scenes.to_tiled(st)).to(dev), n, dt,
                                                  prev=torch.from_numpy(scenes.to_tiled(pv)).to(dev)).cpu().numpy(), n)
    eng.set_prev_velocity(pv)
    F, T = eng.step_wrench_aos(torch.from_numpy(np.ascontiguousarray(st[:, 0:3])).to(dev),
                               torch.from_numpy(np.ascontiguousarray(st[:, [6, 3, 4, 5]])).to(dev),
                               torch.from_numpy(np.ascontiguousarray(st[:, 7:13])).to(dev), dt)
    aos = np.concatenate([F.cpu().numpy(), T.cpu().numpy()], 1)
    assert np.array_equal(soa, til)
    for o in (soa, aos):
        assert ho.wrench_error(o[:, :3], o[:, 3:], rf, rt, pr, rho, g).max() <= GATE
    # back to the default: the reference-executed Numba fixtures again, and different from the Warp result
    eng.set_semantics("numba")
    nb = eng.step_wrench(torch.from_numpy(scenes.to_soa(st)).to(dev), dt, prev=torch.from_numpy(scenes.to_soa(pv)).to(dev)).cpu().numpy().T
    assert ho.wrench_error(nb[:, :3], nb[:, 3:], fx["net_force"], fx["net_torque"], pr, rho, g).max() <= GATE
    assert np.abs(nb - soa).max() > 1e-3
    eng.close()


@pytest.mark.gpu
def test_gpu_components_warp_mode_and_wrapper(native_built):
    import torch
    from silver2_isaacsim_amd.wrapper import HipHydrodynamicsWrapper
    fx = load_golden("c4")
    rho, g = float(fx["rho"]), float(fx["g"])
    st, pr = fx["state"], fx["params"]
    n = len(st)
    acc = ((st[:, 7:13].astype(np.float64) - fx["prev"].astype(np.float64)) / float(fx["dt"])).astype(np.float32)
    ref = ho.solve_components(st, acc, pr, rho, g, semantics="warp")
    w = HipHydrodynamicsWrapper(pr[:, 0], pr[:, 1], pr[:, 2], pr[:, 3], pr[:, 4], pr[:, 5], pr[:, 6], rho, g,
                                pr[:, 8], pr[:, 9], pr[:, 7], device="cuda:0", semantics="warp")
    outs = w.calculate_hydrodynamic_forces(st[:, 0:3], st[:, 3:7], st[:, 7:10], st[:, 10:13], acc[:, :3], acc[:, 3:])
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    vol = pr[:, :3].astype(np.float64).prod(1)
    floor = np.maximum(1e-3 * rho * g * vol, 1e-12)
    for k, name in enumerate(ho.COMPONENT_FIELDS[:6]):
        rel = np.linalg.norm(outs[k] - ref[name], axis=1) / np.maximum(np.linalg.norm(ref[name], axis=1), floor)
        assert rel.max() < 5e-5, name
    dry = ref["ratio"] == 0
    assert dry.any()
    assert np.array_equal(outs[6][dry], st[dry, 0:3]) and np.array_equal(outs[7][dry], st[dry, 0:3])     # N6
    assert np.abs(outs[6] - ref["center_of_buoyancy"]).max() < 3e-5 and np.abs(outs[7] - ref["center_of_pressure"]).max() < 3e-5
    w.close()
    with pytest.raises(ValueError):
        HipHydrodynamicsWrapper(1, 1, 1, 1, 1, 1, 1, 1025.0, 9.81, 0, 0, 0, device="cuda:0", semantics="cuda")


# ---------------------------------------- GPU: the HIP entries against the executed Warp source (warp_reference.npz)
# the smallest shapes that still cover what goes wrong: three full tiles and 8 lanes; two blocks, the last wave with one
# live lane; the same on exact ties; the degenerate-input table
WARP_GPU_SHAPES = [("c4", 200), ("c4", 321), ("ties", 321), ("edge", 81)]


def _wrench_entries(eng, st, pv, dt):
    """{entry: (n,6) net wrench} of the plain SoA, tiled and array-of-structs wrench entries and of one explicit
    step_fused_tiled with its wrench output kept."""
    import torch
    from silver2_isaacsim_amd import scenes
    dev, n = "cuda:0", len(st)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)     # noqa: E731
    out = {}
    out["soa"] = eng.step_wrench(t(scenes.to_soa(st)), dt, prev=t(scenes.to_soa(pv))).cpu().numpy().T
    out["tiled"] = scenes.from_tiled(eng.step_wrench_tiled(t(scenes.to_tiled(st)), n, dt, prev=t(scenes.to_tiled(pv))).cpu().numpy(), n)
    eng.set_prev_velocity(pv.copy())
    F, T = eng.step_wrench_aos(t(st[:, 0:3]), t(st[:, [6, 3, 4, 5]]), t(st[:, 7:13]), dt)
    out["aos"] = np.concatenate([F.cpu().numpy(), T.cpu().numpy()], 1)
    old = np.zeros((n, 13), np.float32)
    old[:, 7:13] = pv
    w = eng.alloc_tiled(6, n)
    eng.step_fused_tiled(t(scenes.to_tiled(st)), t(scenes.to_tiled(old)), n, dt, wrench=w)
    torch.cuda.synchronize()
    out["fused"] = scenes.from_tiled(w.cpu().numpy(), n)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", WARP_GPU_SHAPES)
def test_gpu_wrench_entries_against_the_executed_warp_source(warp_reference, name, n, native_built):
    """Warp mode, fp32 records: every wrench entry inside the 1e-5 gate of the fixture's net wrench on finite & ~hole
    bodies that are not tiny."""
    r = warp_reference[name]
    st, pv, pr = r.state[:n], r.prev[:n], r.params[:n]
    sel = (r.ok & ~r.tiny)[:n]
    assert sel.sum() >= 0.7 * n
    eng = _engine(n, r.rho, r.g, pr.copy(), "f32", "warp")
    try:
        outs = _wrench_entries(eng, st, pv, r.dt)
    finally:
        eng.close()
    assert np.array_equal(outs["soa"], outs["tiled"])
    for entry, o in outs.items():
        with np.errstate(all="ignore"):
            err = r.wrench_error(o[:, :3], o[:, 3:], slice(0, n))
        print(f"[{name}[:{n}] {entry}] {int(sel.sum())} bodies: net wrench max {np.nanmax(np.where(sel, err, 0)):.3e}")
        bad = np.where(sel & ~(err <= GATE))[0]
        assert len(bad) == 0, (name, entry, bad[:5], err[bad[:5]])


@pytest.mark.gpu
def test_gpu_batched_ragged_scenes_against_the_executed_warp_source(warp_reference, native_built):
    """hydro_step_wrench_tiled_batch, Warp mode: c4[:200] and ties[:321] in one launch."""
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.engine import HydroEngine
    cuts = [("c4", 200), ("ties", 321)]
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to("cuda:0")     # noqa: E731
    engines = [_engine(n, warp_reference[name].rho, warp_reference[name].g, warp_reference[name].params[:n].copy(), "f32", "warp")
               for name, n in cuts]
    try:
        states = [t(scenes.to_tiled(warp_reference[name].state[:n])) for name, n in cuts]
        prevs = [t(scenes.to_tiled(warp_reference[name].prev[:n])) for name, n in cuts]
        outs = HydroEngine.step_wrench_tiled_batch(engines, states, warp_reference["c4"].dt, prevs=prevs)
        torch.cuda.synchronize()
        outs = [scenes.from_tiled(o.cpu().numpy(), n) for o, (_, n) in zip(outs, cuts)]
    finally:
        for e in engines:
            e.close()
    assert warp_reference["c4"].dt == warp_reference["ties"].dt
    for o, (name, n) in zip(outs, cuts):
        r = warp_reference[name]
        sel = (r.ok & ~r.tiny)[:n]
        err = r.wrench_error(o[:, :3], o[:, 3:], slice(0, n))
        print(f"[batch {name}[:{n}]] {int(sel.sum())} bodies: net wrench max {np.nanmax(np.where(sel, err, 0)):.3e}")
        assert len(np.where(sel & ~(err <= GATE))[0]) == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", WARP_GPU_SHAPES)
def test_gpu_components_against_the_executed_warp_source(warp_reference, name, n, native_built):
    """step_components and the wrapper's eight tensors, Warp mode, against the fixture's eight outputs with the tolerances
    of test_gpu_components_warp_mode_and_wrapper: the six force / torque vectors to 5e-5 of max(|ref|, 1e-3 rho g V),
    the centres to 3e-5 m - or, where fp32 cannot hold a coordinate that well (the 10 km cases: an ulp of 1e4 is 1e-3),
    to half an fp32 ulp of it; the centres of a body without a wet keypoint are its position, bit for bit (N6; a body
    with wet keypoints and a ratio <= 1e-9 - ties[185] - reports their mean, like the fixture)."""
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.wrapper import HipHydrodynamicsWrapper
    r = warp_reference[name]
    st, pr, ref = r.state[:n], r.params[:n], r.components[:n]
    acc = r.accel[:n].astype(np.float32)
    sel = (r.ok & ~r.tiny)[:n]
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to("cuda:0")     # noqa: E731
    eng = _engine(n, r.rho, r.g, pr.copy(), "f32", "warp")
    try:
        comps, _ = eng.step_components(t(scenes.to_soa(st)), t(scenes.to_soa(acc)))
        torch.cuda.synchronize()
        got = {"step_components": comps.cpu().numpy().T.reshape(n, 8, 3)}
    finally:
        eng.close()
    st, pr = st.copy(), pr.copy()                                     # (the shared reference is read-only)
    w = HipHydrodynamicsWrapper(pr[:, 0], pr[:, 1], pr[:, 2], pr[:, 3], pr[:, 4], pr[:, 5], pr[:, 6], r.rho, r.g,
                                pr[:, 8], pr[:, 9], pr[:, 7], device="cuda:0", semantics="warp")
    try:
        outs = w.calculate_hydrodynamic_forces(st[:, 0:3], st[:, 3:7], st[:, 7:10], st[:, 10:13], acc[:, :3], acc[:, 3:])
        torch.cuda.synchronize()
        got["wrapper"] = np.stack([o.cpu().numpy() for o in outs], axis=1)
    finally:
        w.close()
    assert np.array_equal(got["wrapper"], got["step_components"])
    vol = pr[:, :3].astype(np.float64).prod(1)
    floor = np.maximum(1e-3 * r.rho * r.g * vol, 1e-12)
    dry = sel & ((r.oracle["branches"][:n] & ((1 << 27) - 1)) == 0)         # no keypoint below the surface
    for entry, c in got.items():
        for k, field in enumerate(ho.COMPONENT_FIELDS[:6]):
            rel = np.linalg.norm(c[:, k] - ref[:, k], axis=1) / np.maximum(np.linalg.norm(ref[:, k], axis=1), floor)
            assert np.all(rel[sel] < 5e-5), (entry, field, np.where(sel & ~(rel < 5e-5))[0][:5])
        for k in (6, 7):
            tol = np.maximum(3e-5, 0.5 * np.spacing(np.abs(ref[:, k]).astype(np.float32)).astype(np.float64) * (1 + 1e-6))
            assert np.all((np.abs(c[:, k] - ref[:, k]) < tol)[sel]), (entry, ho.COMPONENT_FIELDS[k])
            assert np.array_equal(c[dry, k], st[dry, 0:3])
    assert dry.any()


@pytest.mark.gpu
def test_gpu_wrench_entries_warp_mode_f16_coefficients(warp_reference, native_built):
    """fp16 records once, on c4[:321]: the fixture is of the fp32 coefficients, so the reference here is the oracle's Warp
    branch - held to the fixture above - on the coefficients as the engine rounds them."""
    from wrench_ulps import f16_params
    r = warp_reference["c4"]
    n = 321
    st, pv, pr = r.state[:n], r.prev[:n], r.params[:n]
    rf, rt, _ = ho.step_wrench(st, pv, f16_params(pr), r.rho, r.g, r.dt, semantics="warp")
    eng = _engine(n, r.rho, r.g, pr.copy(), "f16", "warp")
    try:
        outs = _wrench_entries(eng, st, pv, r.dt)
    finally:
        eng.close()
    sel = (r.ok & ~r.tiny)[:n]
    for entry, o in outs.items():
        err = ho.wrench_error(o[:, :3], o[:, 3:], rf, rt, pr, r.rho, r.g)
        print(f"[c4[:321] f16 {entry}] net wrench max {err[sel].max():.3e}")
        assert err[sel].max() <= GATE, entry
