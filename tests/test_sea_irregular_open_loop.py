"""The spectrum, the ensemble and the finite-depth sea in the open-loop entries (hydro_step_wrench_tiled_irr,
hydro_step_wrench_aos_irr) and in the plugin, as far as a machine without a GPU can see them: the C boundary, the Python host's
marshalling against the stand-in library, which symbol a prepared step issues for each of the five engine states, the plugin's
calls with a fake engine, the "spectrum" object of the JSON "sea" block, the generated code's budget - and the condition, on the
fp64 reference alone, that makes the identities of tests/test_sea_irregular_open_loop_gpu.py mean something."""
import ctypes
import json
import logging
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import irregular_open_loop_cases as ic
import sea_ensemble_harness as seh
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import behavior as hb
from silver2_isaacsim_amd import build as hbuild
from silver2_isaacsim_amd import config as cfg
from silver2_isaacsim_amd.sea import jonswap, pierson_moskowitz, SeaEnsemble, SeaSpectrum, SeaState
from silver2_isaacsim_amd.testing import build_main_scene
from designed_populations import hold_pop  # noqa: F401  (fixtures are requested by name)
from engine_stand_ins import DT, eng, F, H, KE, lib, N, O, ORI, P6, POS, PREVS, refused, S, STREAM, T, TILES, TQ, VELS  # noqa: F401

SIBLINGS = {"hydro_step_wrench_tiled_irr": "hydro_step_wrench_tiled_sea", "hydro_step_wrench_aos_irr": "hydro_step_wrench_aos_sea"}
W = T((TILES, 4, 64), 0x98000000)                                 # the sample's output


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    for name, sibling in SIBLINGS.items():
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
        assert proto(name) == proto(sibling)                      # exactly the _sea sibling's prototype
        assert nat.SIGNATURES[name][0] is nat.SIGNATURES[sibling][0] and nat.SIGNATURES[name][1] == nat.SIGNATURES[sibling][1]
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    para = text[text.index("/* Irregular sea in the open-loop steps"):]
    para = para[:para.index("*/")]
    for phrase in ("hydro_sea_spectrum_sample, hydro_sea_ensemble_sample", "hydro_sea_finite_depth_sample with (step_index = 1, dt = time)", "step_index = 0",
                   "TRUE velocity", "NOT COVERED", "hydro_step_wrench_tiled_ke", "hydro_step_wrench_tiled_batch", "hydro_step_wrench[_ext]",
                   "hydro_step_components[_aos]", "time > 2^52", "ceil(tiles(n) / tiles_per_sea) > count", "an ensemble of one member",
                   "EVERY EXISTING ENTRY BEHAVES AS BEFORE", "DESIGN.md section 33"):
        assert phrase in para, phrase
    # the sentences that said who knows a spectrum, an ensemble and a finite-depth sea now name these entries as well
    for sentence in ("entries below hydro_step_fused_tiled_multi_bed ignore the bed.", "as every entry but hydro_step_fused_tiled_multi_irr and _stat ignores a spectrum.",
                     "EVERY OTHER ENTRY IGNORES A FINITE-DEPTH SEA."):
        after = text[text.index(sentence) + len(sentence):][:400]
        assert "hydro_step_wrench_tiled_irr and hydro_step_wrench_aos_irr" in " ".join(after.replace("*", " ").split()), sentence


def test_the_calls_are_plain_c(tmp_path):
    """Both calls through a C99 compiler at its strictest (compiled, not linked: the prototypes are what is checked)."""
    src = tmp_path / "calls.c"
    src.write_text('#include <stddef.h>\n#include "hydro.h"\n'
                   "int calls(hydro_t *h, const float *in, float *out) {\n"
                   "  int rc = hydro_step_wrench_tiled_irr(h, 64, in, 832, NULL, 0, 1.0 / 60.0, out, 384, 2.5, NULL);\n"
                   "  rc += hydro_step_wrench_tiled_irr(h, 64, in, 832, in, 384, 1.0 / 60.0, out, 384, 0.0, NULL);\n"
                   "  rc += hydro_step_wrench_aos_irr(h, 64, in, in, 1, in, 1.0 / 60.0, out, out, 2.5, NULL);\n"
                   "  return rc; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", str(tmp_path / "calls.o"),
                    str(src)], check=True)


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in SIBLINGS:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    assert lib_.hydro_step_wrench_tiled_irr(None, 64, None, 832, None, 384, 1 / 60, None, 384, 0.5, None) == nat.HYDRO_E_ARG == -1
    assert lib_.hydro_step_wrench_aos_irr(None, 64, None, None, 0, None, 1 / 60, None, None, 0.5, None) == -1
    assert lib_.hydro_step_wrench_aos_irr(None, 64, None, None, 0, None, 1 / 60, None, None, float("nan"), None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
# the five engine states, as the host reaches them, and the symbol a prepared step issues for a `time` in each
SPEC = SeaSpectrum((0.1, 0.0, 0.0)).add_wave(0.2, 0.3, 0.0, 1.7, 0.1)
STATES = {
    "fd": (lambda e: e.set_sea_finite_depth(SeaSpectrum((0.1, 0.0, 0.0), depth=9.0).add_wave(0.2, 0.3, 0.0, 1.7, 0.1)), "_irr"),
    "ensemble": (lambda e: e.set_sea_ensemble(SeaEnsemble([SPEC, SPEC], 512)), "_irr"),
    "spectrum": (lambda e: e.set_sea_spectrum(SPEC), "_irr"),
    "sea": (lambda e: e.set_sea(SeaState((0.3, 0.0, 0.0))), "_sea"),
    "none": (lambda e: None, "_sea"),
}


def _enter(eng, lib, state):
    STATES[state][0](eng)
    lib.calls.clear()
    return STATES[state][1]


@pytest.mark.parametrize("prev,prev_args", PREVS)
def test_step_wrench_tiled_irr(lib, eng, prev, prev_args):
    head = (H, 1000, 0x10000000, 832) + prev_args + (0.01, 0x40000000, 384)
    assert eng.step_wrench_tiled_irr(S, N, DT, 2.5, out=O, prev=prev, stream=STREAM) is O
    assert lib.calls == [("hydro_step_wrench_tiled_irr", head + (2.5, STREAM))]       # `time` stands in front of the stream
    lib.calls.clear()
    eng.step_wrench_tiled_irr(S, N, DT, 7.0, O, prev, STREAM)                         # (state, n, dt, time, out, prev, stream)
    assert lib.calls == [("hydro_step_wrench_tiled_irr", head + (7.0, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.step_wrench_tiled_irr, O, N, DT, 1.0, out=O, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.step_wrench_tiled_irr, S, N, DT, 1.0, out=S, stream=STREAM)


@pytest.mark.parametrize("state", list(STATES))
def test_prepared_tiled_step_issues_the_symbol_of_the_engine_state(lib, eng, state):
    suffix = _enter(eng, lib, state)
    head = (H, 1000, 0x10000000, 832, 0x20000000, 384, 0.01, 0x40000000, 384)
    parent = ("hydro_step_wrench_tiled", head + (STREAM,))
    step = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=STREAM)
    assert lib.calls == []
    assert step() is O and step(None) is O and step(2.5) is O and step(time=0.0) is O and step() is O
    timed = "hydro_step_wrench_tiled" + suffix
    assert lib.calls == [parent, parent, (timed, head + (2.5, STREAM)), (timed, head + (0.0, STREAM)), parent]     # time=None: today's call
    # the state is asked at every step: the same prepared step follows a sea set or cleared later
    lib.calls.clear()
    eng.set_sea(None); eng.set_sea_spectrum(None); eng.set_sea_ensemble(None); eng.set_sea_finite_depth(None)
    lib.calls.clear()
    step(1.0)
    eng.set_sea_spectrum(SPEC)
    step(1.0)
    assert [c[0] for c in lib.calls] == ["hydro_step_wrench_tiled_sea", "hydro_set_sea_spectrum", "hydro_step_wrench_tiled_irr"]
    lib.calls.clear()
    with_ke = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=STREAM, ke_out=KE)
    refused(lib, "the sea entry does not sample the kinetic energy (prepared with ke_out)", with_ke, 1.0)


@pytest.mark.parametrize("q", [False, True])
def test_step_wrench_aos_irr(lib, eng, q):
    head, out = (H, 1000, 0x70000000, 0x71000000, int(q), 0x72000000), (0x73000000, 0x74000000)
    assert eng.step_wrench_aos_irr(POS, ORI, VELS, DT, 3.25, F, TQ, quat_xyzw=q, stream=STREAM) == (F, TQ)
    assert lib.calls == [("hydro_step_wrench_aos_irr", head + (0.01,) + out + (3.25, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (1000,6) tensor on cuda:0", eng.step_wrench_aos_irr, POS, ORI, T((N - 1, 6), 0x1000), DT, 1.0, F, TQ,
            stream=STREAM)


@pytest.mark.parametrize("state", list(STATES))
def test_prepared_rows_step_issues_the_symbol_of_the_engine_state(lib, eng, state):
    suffix = _enter(eng, lib, state)
    head, out = (H, 1000, 0x70000000, 0x71000000, 0, 0x72000000), (0x73000000, 0x74000000)
    timed = lambda dt, t: ("hydro_step_wrench_aos" + suffix, head + (dt,) + out + (t, STREAM))  # noqa: E731
    parent = lambda dt: ("hydro_step_wrench_aos", head + (dt,) + out + (STREAM,))  # noqa: E731
    step = eng.prepare_step_wrench_aos(POS, ORI, VELS, F, TQ)
    assert lib.calls == []
    assert step(DT, STREAM) == (F, TQ) and step(DT, STREAM, None) == (F, TQ) and step(DT, STREAM, 0.0) == (F, TQ)
    assert step(0.02, stream=STREAM, time=0.01) == (F, TQ) and step(0.02, STREAM) == (F, TQ)
    assert lib.calls == [parent(0.01), parent(0.01), timed(0.01, 0.0), timed(0.02, 0.01), parent(0.02)]


def test_a_cleared_kind_leaves_the_one_that_is_still_set(lib, eng):
    """Clearing with None is always allowed, also of a kind that is not set: what the engine holds decides."""
    eng.set_sea_finite_depth(SeaSpectrum((0.1, 0.0, 0.0), depth=9.0))
    eng.set_sea_spectrum(None)
    assert eng.holds_irregular_sea()
    eng.set_sea_finite_depth(None)
    assert not eng.holds_irregular_sea()
    eng.set_sea(SeaState((0.3, 0.0, 0.0)))
    assert not eng.holds_irregular_sea()


@pytest.mark.parametrize("state,symbol", [("fd", "hydro_sea_finite_depth_sample"), ("ensemble", "hydro_sea_ensemble_sample"),
                                          ("spectrum", "hydro_sea_spectrum_sample")])
def test_irregular_sea_sample_at(lib, eng, state, symbol):
    """time 0 -> step index 0 (any dt > 0), time t -> (1, t): (double)1 * t == t exactly; the sample is the kind's own."""
    _enter(eng, lib, state)
    assert eng.irregular_sea_sample_at(S, N, 0.0, out=W, stream=STREAM) is W
    assert eng.irregular_sea_sample_at(S, N, 16666.666666666668, out=W, stream=STREAM) is W
    assert eng.irregular_sea_sample_at(S, N, 5e-324, out=W, stream=STREAM) is W
    (n0, a0), (n1, a1), (n2, a2) = lib.calls
    assert n0 == n1 == n2 == symbol
    assert a0[:5] == (H, 1000, 0x10000000, 832, 0) and a0[5] > 0.0 and a0[6:] == (0x98000000, 256, STREAM)
    assert a1 == (H, 1000, 0x10000000, 832, 1, 16666.666666666668, 0x98000000, 256, STREAM)
    assert a2[4:6] == (1, 5e-324)


# ---- the plugin, with a fake engine ----------------------------------------------------------------------------------------------
class FakeEngine:
    """Records what the plugin asks of an engine; nothing runs.  `built` lists the engines in the order they were made."""
    built: list = []

    def __init__(self, capacity, device, rho, g):
        self.device, self.n, self.capacity, self.calls = torch.device("cpu"), capacity, capacity, []
        FakeEngine.built.append(self)

    def set_params(self, rows):
        self.n = len(rows)

    def set_semantics(self, semantics):
        pass

    def sync(self):
        self.calls.append(("sync",))

    def set_sea(self, sea):
        self.calls.append(("set_sea", sea))

    def set_sea_spectrum(self, sea):
        self.calls.append(("set_sea_spectrum", sea))

    def set_sea_finite_depth(self, sea, n=None):
        self.calls.append(("set_sea_finite_depth", sea) + (() if sea is None else (n,)))

    def get_prev_velocity(self):
        return torch.zeros((6, self.n))

    def set_prev_velocity(self, prev):
        self.calls.append(("set_prev_velocity",))

    def close(self):
        self.calls.append(("close",))

    def prepare_step_wrench_aos(self, positions, orientations, velocities, forces=None, torques=None, quat_xyzw=False):
        self.calls.append(("prepare",))

        def step(*args, **kw):
            self.calls.append(("step",) + args + tuple(sorted(kw.items())))
            forces.zero_(); torques.zero_()
            return forces, torques
        return step


@pytest.fixture
def fake(monkeypatch):
    hb.REGISTRY.clear()
    FakeEngine.built = []
    monkeypatch.setattr(hb, "HydroEngine", FakeEngine)
    yield FakeEngine
    hb.REGISTRY.clear()


SEA = SeaState.regular(0.4, 8.0, 30.0, current=(0.3, -0.1, 0.0))
JONSWAP = jonswap(1.2, 7.0, 25.0, components=16, seed=5, current=(0.2, 0.0, 0.0))
SHALLOW = jonswap(1.2, 7.0, 25.0, components=16, seed=5, current=(0.2, 0.0, 0.0), depth=9.0)
DTS = (1.0 / 60.0, 0.02, 1.0 / 90.0, 0.013)
MODES = pytest.mark.parametrize("batched", [True, "callbacks", False], ids=["scene", "callbacks", "per-prim"])


def _scene(batched, **kw):
    world, host, prims, behaviors = build_main_scene(batched=batched, device="cpu", **kw)
    for b in behaviors:
        b.on_play()
    return world, host, behaviors


def _sums(dts):
    out, t = [], 0.0
    for dt in dts:
        out.append(t)
        t = t + dt
    return out


def _set(sea, capacity):
    return ("set_sea_finite_depth", sea, capacity) if sea.depth is not None else ("set_sea_spectrum", sea)


@MODES
@pytest.mark.parametrize("sea", [JONSWAP, SHALLOW], ids=["spectrum", "depth"])
def test_with_a_spectrum_the_times_are_the_sums_of_the_earlier_deltas(fake, batched, sea):
    _, host, behaviors = _scene(batched)
    hb.HydrodynamicsBehavior.set_sea(sea)                        # before any engine exists
    for dt in DTS[:3]:
        host.step(dt)
    want = [("step", dt, None, t) for dt, t in zip(DTS[:3], _sums(DTS[:3]))]
    assert [w[3] for w in want] == [0.0, DTS[0], DTS[0] + DTS[1]] and len({DTS[0], DTS[1], DTS[2]}) == 3
    assert len(fake.built) == (20 if batched is False else 1)
    for e in fake.built:
        assert e.calls == [("prepare",), ("sync",), _set(sea, e.capacity)] + want
    assert behaviors[3].sea_time == (DTS[0] + DTS[1]) + DTS[2]


@MODES
def test_changing_the_kind_clears_the_old_one_before_setting_the_new(fake, batched):
    _, host, behaviors = _scene(batched)
    host.step(DTS[0])                                            # engines exist, no sea
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[1])
    behaviors[0].set_sea(JONSWAP)
    host.step(DTS[2])
    hb.HydrodynamicsBehavior.set_sea(SHALLOW)
    host.step(DTS[3])
    hb.HydrodynamicsBehavior.set_sea(None)
    host.step(DTS[0])
    host.step(DTS[1])
    t = _sums(DTS + DTS[:2])
    for e in fake.built:
        assert e.calls == [("prepare",), ("step", DTS[0]),
                           ("sync",), ("set_sea", SEA), ("step", DTS[1], None, t[1]),
                           ("sync",), ("set_sea", None), ("set_sea_spectrum", JONSWAP), ("step", DTS[2], None, t[2]),
                           ("sync",), ("set_sea_spectrum", None), ("set_sea_finite_depth", SHALLOW, e.capacity), ("step", DTS[3], None, t[3]),
                           ("sync",), ("set_sea_finite_depth", None), ("step", DTS[0]), ("step", DTS[1])]
    assert behaviors[0].sea_time == t[5] + DTS[1]                 # the clock was never touched


@MODES
def test_a_sea_state_and_no_sea_give_todays_call_sequences(fake, batched):
    _, host, behaviors = _scene(batched)
    for dt in DTS[:2]:
        host.step(dt)
    for e in fake.built:
        assert e.calls == [("prepare",), ("step", DTS[0]), ("step", DTS[1])]
    other = SeaState((0.0, 0.2, 0.0))
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[2])
    behaviors[0].set_sea(other)
    host.step(DTS[3])
    hb.HydrodynamicsBehavior.set_sea(None)
    host.step(DTS[0])
    t = _sums(DTS)
    for e in fake.built:
        assert e.calls[3:] == [("sync",), ("set_sea", SEA), ("step", DTS[2], None, t[2]), ("sync",), ("set_sea", other), ("step", DTS[3], None, t[3]),
                               ("sync",), ("set_sea", None), ("step", DTS[0])]


def test_an_ensemble_is_refused(fake):
    ens = SeaEnsemble([JONSWAP, JONSWAP], 64)
    hb.HydrodynamicsBehavior.set_sea(JONSWAP)
    for setter in (hb.HydrodynamicsBehavior.set_sea, hb.REGISTRY.set_sea):
        with pytest.raises(ValueError, match="a scene has one sea"):
            setter(ens)
    assert hb.REGISTRY.sea is JONSWAP                             # what was set stays


# ---- the JSON block ----------------------------------------------------------------------------------------------------------------
def _config(tmp_path, sea, gravity=9.81):
    data = cfg.default_config()
    data["globals"]["gravity"] = gravity
    data["sea"] = sea
    path = os.path.join(tmp_path, cfg.CONFIG_FILE_NAME)
    json.dump(data, open(path, "w"))
    return path


@pytest.mark.parametrize("extra,direct", [
    ({"kind": "jonswap", "gamma": 2.5, "components": 24, "seed": 9, "spread": "cos2", "depth": 12.0},
     lambda g: jonswap(1.5, 7.0, 40.0, gamma=2.5, components=24, seed=9, spread="cos2", depth=12.0, current=(0.3, -0.1, 0.0), g=g)),
    ({"kind": "jonswap"}, lambda g: jonswap(1.5, 7.0, 40.0, current=(0.3, -0.1, 0.0), g=g)),
    ({"kind": "pierson_moskowitz", "components": 10}, lambda g: pierson_moskowitz(1.5, 7.0, 40.0, components=10, current=(0.3, -0.1, 0.0), g=g)),
], ids=["jonswap-all-keys", "jonswap-defaults", "pierson-moskowitz"])
def test_json_block_sets_the_spectrum_with_the_files_gravity(fake, tmp_path, extra, direct):
    block = {"current": [0.3, -0.1, 0.0], "spectrum": dict({"hs": 1.5, "tp": 7.0, "heading_deg": 40.0}, **extra)}
    build_main_scene(config_path=_config(tmp_path, block, gravity=9.8), device="cpu")
    sea, want = hb.REGISTRY.sea, direct(9.8)
    assert isinstance(sea, SeaSpectrum) and sea.current == (0.3, -0.1, 0.0) and sea.depth == want.depth
    assert sea.waves == want.waves and len(sea.waves) == extra.get("components", 64)      # the constants of a direct call, the FILE's gravity
    assert sea.waves != direct(9.81).waves


@pytest.mark.parametrize("block", [
    {"waves": [{"height": 0.4, "period": 8.0}], "spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0}},     # both
    {"spectrum": {"kind": "bretschneider", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0}},
    {"spectrum": {"kind": "jonswap", "tp": 7.0, "heading_deg": 0.0}},                                                           # no hs
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0}},                                                                    # no heading
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": -7.0, "heading_deg": 0.0}},
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0, "components": 65}},
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0, "depth": 0.0}},
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0, "swell": 1}},
    {"spectrum": {"kind": "pierson_moskowitz", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0, "gamma": 3.3}},
    {"spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0, "spread": "cos4"}},
    {"spectrum": ["jonswap", 1.0, 7.0]},
    {"current": [0.1, 0.2], "spectrum": {"kind": "jonswap", "hs": 1.0, "tp": 7.0, "heading_deg": 0.0}},
])
def test_a_malformed_spectrum_block_is_logged_and_ignored(fake, tmp_path, caplog, block):
    with caplog.at_level(logging.ERROR, logger="silver2_isaacsim_amd"):
        _, host, prims, _ = build_main_scene(config_path=_config(tmp_path, block), device="cpu")
    assert hb.REGISTRY.sea is None and hb.REGISTRY._sea_source is None
    assert any("[Hydro] JSON Error" in r.getMessage() for r in caplog.records)
    body = next(p for p in prims if p.GetName() == "Body")       # the rest of the file was applied
    assert host.get_exposed_variable(body, cfg.full_attr_name("liftCoefficient")) == 0.5


# ---- the generated code ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "hydro.s")
    cmd = [hbuild.hipcc_path()] + hbuild.device_flags() + ["--cuda-device-only", "-S", "-o", out, hbuild.SRC]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(out))
    assert res.returncode == 0, res.stderr[-3000:]
    return open(out).read()


def _loops(body):
    """The loops of a function's text: the lines from a label to a branch back to it."""
    lines = body.splitlines()
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i + 1) <= i:
            out.append([re.match(r"\s+([a-z][a-z0-9_]+)", x).group(1) for x in lines[labels[m.group(1)]:i + 1] if re.match(r"\s+[a-z]", x)])
    return out


def test_new_kernels_stay_inside_the_open_loop_budget(assembly):
    """Every instantiation: no scratch, no LDS, registers for four waves per SIMD; and the component loops read the table with
    scalar loads in every trip, with no vector-memory or LDS instruction in them."""
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", assembly, re.S)}
    tiled = {k: d for k, d in desc.items() if "wrench_tiled_irr_kernel" in k}
    rows = {k: d for k, d in desc.items() if "wrench_aos_irr_kernel" in k}
    assert len(tiled) == 32 and len(rows) == 16                   # <HALF, ENGINE_PREV, NT, WARP, DEPTH> and <HALF, NT, WARP, DEPTH>
    worst = 0
    for name, d in {**tiled, **rows}.items():
        assert int(d["private_segment_fixed_size"]) == 0 and int(d.get("group_segment_fixed_size", 0)) == 0, name
        assert int(d["next_free_vgpr"]) <= 128, (name, d["next_free_vgpr"])
        worst = max(worst, int(d["next_free_vgpr"]))
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)s_endpgm", assembly, re.S | re.M).group(1)
        loops = _loops(body)
        assert len(loops) == 4, (name, len(loops))                # two passes over the components: groups of four, and the remainder
        for ins in loops:
            assert any(i.startswith("s_load_dword") for i in ins), name
            assert not any(i.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")) for i in ins), name
    print(f"[open-loop irregular sea] 48 instantiations, at most {worst} VGPRs, no scratch, no LDS")


# ---- the condition that makes the device identities mean something -----------------------------------------------------------------
def test_on_the_fp64_reference_the_sea_moves_nearly_every_body_and_so_does_the_depth(hold_pop):
    """For the populations and the seas of the GPU module: the fp64 wrench in the irregular sea differs from the still-water wrench on
    at least 3 in 4 bodies and on some body of every tile; at h = 9 m the finite-depth wrench differs from the deep one on at least
    3 in 4 bodies.  "Differs": by more than ten times the gate the device is held to (irregular_open_loop_cases.MOVED)."""
    st, pv, params = ic.near_surface(*hold_pop[:3])
    pr = params["f32"]
    assert (np.abs(st[:, 2]) <= 2.0).all() and len(st) == ic.N == 321
    low = {"sea": 1.0, "depth": 1.0}
    for time in ic.TIMES:
        still = ic.fp64_wrench(None, st, pv, pr, time)
        cases = [(ic.lone(count), n) for count in ic.COUNTS for n in ic.SIZES] + [(seh.ensemble(count, n, tps), n) for count in (11, 64)
                                                                                  for n, tps in ic.ENSEMBLE_CASES]
        cache = {}
        for sea, n in cases:
            key = (id(sea) if hasattr(sea, "members") else len(sea.waves), n if hasattr(sea, "members") else 0)
            if key not in cache:
                m = ic.N if not hasattr(sea, "members") else n
                cache[key] = (ic.fp64_wrench(sea, st[:m], pv[:m], pr, time), ic.fp64_wrench(ic.at_depth(sea), st[:m], pv[:m], pr, time))
            deep, shallow = (w[:n] for w in cache[key])
            for got, base, what in ((deep, still[:n], "sea"), (shallow, still[:n], "sea"), (shallow, deep, "depth")):
                fraction, every_tile = ic.moved(got, base, pr)
                low[what] = min(low[what], fraction)
                assert fraction >= 0.75 and (every_tile or what == "depth"), (what, time, n, fraction, every_tile)
    print(f"[fp64 condition] smallest fraction of bodies moved: by the sea {low['sea']:.3f}, by the depth of 9 m {low['depth']:.3f}")
