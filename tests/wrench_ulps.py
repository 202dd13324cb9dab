"""Shared by tests/test_wrench_metric.py (CPU) and tests/test_wrench_ulps_gpu.py: the populations on which every wrench is
held to its correctly rounded value, their longdouble references, and the check itself (hydro_oracle.wrench_error_ulps).

A reference is evaluated in np.longdouble (x87, 64-bit mantissa) AND in fp64; a body on which the two take a different
decision of the model (hydro_oracle.branch_flips) has no well-defined "correct rounding" and is compared with the 1e-5
gate of SURVEY.md 8d instead.  How many such bodies each population has is part of the test (EXPECTED_FLIPS)."""
import importlib.util
import os

import numpy as np

import populations as pop
from conftest import REPO, load_golden
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import scenes

GATE = 1e-5
# golden fixtures with fp32-exact inputs ("kat" holds fp64 numbers: handing them to an fp32 interface rounds the inputs)
FIXTURES = ("c2", "c3", "c4", "c5", "c4_adversarial", "ties")
CONDITIONING = {"terminal_rise_100x": lambda: pop.terminal_rise(cancel=100.0),
                "terminal_rise_300x": lambda: pop.terminal_rise(seed=13, cancel=300.0),
                "floaters_0.5deg": lambda: pop.near_upright_floaters(),
                "floaters_0.05deg": lambda: pop.near_upright_floaters(seed=14, tilt_deg=0.05),
                "torque_balance_300x": lambda: pop.torque_balance(),
                "torque_balance_3000x": lambda: pop.torque_balance(seed=16, cancel=3000.0)}
# bodies whose fp64 and longdouble references decide a branch differently.  `ties` holds quantised bodies with exact
# ties on purpose; on its non-unit quaternions (0.25, 0.25, 0.25, 0.75) a face alignment that is exactly 0 comes out as
# +-1e-17 in fp64, so that face's `take` differs (its area share is ~1e-17 either way).  Every other population is
# branch-margin gated or random, and has none.
EXPECTED_FLIPS = {"ties": 13}


def _stress(n=65536, seed=1):
    spec = importlib.util.spec_from_file_location("extreme_ranges", os.path.join(REPO, "tests", "tools", "extreme_ranges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.population(n, seed)


def population(name):
    """(state, prev, params, rho, g, dt) of a named population, fp32 arrays."""
    if name in FIXTURES:
        fx = load_golden(name)
        return fx["state"], fx["prev"], fx["params"], float(fx["rho"]), float(fx["g"]), float(fx["dt"])
    if name in CONDITIONING:
        st, pv, pr = CONDITIONING[name]()
        return st, pv, pr, pop.RHO, pop.G, pop.DT
    if name == "stress":
        st, pv, pr, dt = _stress()
        return st, pv, pr, pop.RHO, pop.G, dt
    if name in ("c4_131072", "c4_131072_ungated"):
        sc = scenes.scene_c4(n=131072, seed=4242, margin=None if name.endswith("ungated") else 1e-4)
        return sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt
    raise KeyError(name)


def f16_params(params):
    """The record as an f16 engine holds it: the seven coefficients rounded to half (the mass and dims stay fp32)."""
    p = np.array(params, dtype=np.float32)
    p[:, 3:10] = p[:, 3:10].astype(np.float16).astype(np.float32)
    return p


class Reference:
    """The longdouble and fp64 references of one population under one semantics / coefficient format."""

    def __init__(self, state, prev, params, rho, g, dt, semantics="numba"):
        self.state, self.prev, self.params, self.rho, self.g, self.dt = state, prev, params, rho, g, dt
        self.ld = ho.step_wrench(state, prev, params, rho, g, dt, semantics, dtype=np.longdouble)
        self.f64 = ho.step_wrench(state, prev, params, rho, g, dt, semantics)
        self.flips = ho.branch_flips(self.f64[2], self.ld[2])

    def head(self, n):
        """The first n bodies (a reference is per body: slicing it is the reference of the slice)."""
        r = Reference.__new__(Reference)
        r.state, r.prev, r.params, r.rho, r.g, r.dt = self.state[:n], self.prev[:n], self.params[:n], self.rho, self.g, self.dt
        r.ld = (self.ld[0][:n], self.ld[1][:n], {k: v[:n] for k, v in self.ld[2].items()})
        r.f64 = (self.f64[0][:n], self.f64[1][:n], {k: v[:n] for k, v in self.f64[2].items()})
        r.flips = {i: v for i, v in self.flips.items() if i < n}
        return r


def check(label, f, t, ref, clamp_bound=ho.CLAMP_ULP_BOUND, expected_flips=None):
    """Hold a wrench (f, t: (N,3) fp32) to the longdouble reference component by component; bodies with a branch flip to
    the 1e-5 gate.  Returns (max over non-clamped bodies, max over clamped bodies, clamped count, flip count)."""
    f, t = np.asarray(f), np.asarray(t)
    assert np.isfinite(f).all() and np.isfinite(t).all(), label
    e = ho.wrench_error_ulps(f, t, ref.ld, ref.state[:, 0:3])
    worst = np.maximum(e["force"], e["torque"])
    flipped = np.zeros(len(f), bool)
    flipped[list(ref.flips)] = True
    if expected_flips is not None:
        assert flipped.sum() == expected_flips, (label, sorted(ref.flips.items())[:5])
    if flipped.any():
        old = ho.wrench_error(f[flipped], t[flipped], ref.f64[0][flipped], ref.f64[1][flipped], ref.params[flipped],
                              ref.rho, ref.g)
        assert old.max() <= GATE, (label, old.max())
    plain, clamped = ~flipped & ~e["clamped"], ~flipped & e["clamped"]
    m_plain = float(worst[plain].max()) if plain.any() else 0.0
    m_clamp = float(worst[clamped].max()) if clamped.any() else 0.0
    bad = np.nonzero(plain & (worst > ho.WRENCH_ULP_BOUND))[0]
    assert bad.size == 0, (f"{label}: {bad.size} non-clamped bodies above {ho.WRENCH_ULP_BOUND}, max {m_plain:.4g} "
                           f"(first {bad[:5].tolist()}: force {e['force'][bad[:5]]}, torque {e['torque'][bad[:5]]})")
    assert m_clamp <= clamp_bound, f"{label}: clamp-active max {m_clamp:.4g} > {clamp_bound}"
    return m_plain, m_clamp, int(clamped.sum()), int(flipped.sum())
