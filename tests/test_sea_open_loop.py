"""The sea in the open-loop entries (hydro_step_wrench_tiled_sea, hydro_step_wrench_aos_sea) and in the plugin, as far as a
machine without a GPU can see it: the C boundary, the Python host's marshalling (the stand-ins of tests/test_engine_calls.py),
the plugin's clock and its calls with a fake engine on an in-memory host, and the "sea" block of the JSON configuration."""
import ctypes
import json
import logging
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import behavior as hb
from silver2_isaacsim_amd import config as cfg
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.testing import build_main_scene
from engine_stand_ins import DT, eng, F, H, KE, lib, N, O, ORI, P6, POS, PREVS, refused, S, STREAM, T, TILES, TQ, VELS  # noqa: F401  (fixtures are requested by name)

ENTRIES = ("hydro_step_wrench_tiled_sea", "hydro_step_wrench_aos_sea")
PARENTS = {"hydro_step_wrench_tiled_sea": "hydro_step_wrench_tiled", "hydro_step_wrench_aos_sea": "hydro_step_wrench_aos"}
W = T((TILES, 4, 64), 0x98000000)                                 # the sample's output


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    for name, parent in PARENTS.items():
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
        # the parent's argument list with `double time` in front of the stream, in the header and in the binding
        assert proto(name) == proto(parent).replace(", void *stream", ", double time, void *stream")
        sea, par = nat.SIGNATURES[name], nat.SIGNATURES[parent]
        assert sea[0] is par[0] and sea[1] == par[1][:-1] + [ctypes.c_double] + par[1][-1:]
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    # the identity with hydro_sea_sample, what the engine's record receives, and what is not covered
    for phrase in ("hydro_sea_sample(step_index = 1, dt = time)", "step_index = 0", "TRUE velocity", "NOT COVERED", "hydro_step_wrench_tiled_ke",
                   "hydro_step_wrench_tiled_batch", "hydro_step_wrench[_ext]", "hydro_step_components[_aos]", "time > 2^52"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    assert lib_.hydro_step_wrench_tiled_sea(None, 64, None, 832, None, 384, 1 / 60, None, 384, 0.5, None) == nat.HYDRO_E_ARG == -1
    assert lib_.hydro_step_wrench_aos_sea(None, 64, None, None, 0, None, 1 / 60, None, None, 0.5, None) == -1
    assert lib_.hydro_step_wrench_aos_sea(None, 64, None, None, 0, None, 1 / 60, None, None, float("nan"), None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prev,prev_args", PREVS)
def test_step_wrench_tiled_sea(lib, eng, prev, prev_args):
    head = (H, 1000, 0x10000000, 832) + prev_args + (0.01, 0x40000000, 384)
    sea, parent = ("hydro_step_wrench_tiled_sea", head + (2.5, STREAM)), ("hydro_step_wrench_tiled", head + (STREAM,))
    assert eng.step_wrench_tiled_sea(S, N, DT, 2.5, out=O, prev=prev, stream=STREAM) is O
    assert lib.calls == [sea]                                    # `time` stands in front of the stream
    lib.calls.clear()
    step = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=prev, stream=STREAM)
    assert lib.calls == []
    assert step() is O and step(None) is O and step(2.5) is O and step(time=0.0) is O and step() is O
    assert lib.calls == [parent, parent, sea, ("hydro_step_wrench_tiled_sea", head + (0.0, STREAM)), parent]


def test_step_wrench_tiled_sea_positional_order_and_refusals(lib, eng):
    """(state, n, dt, time, out, prev, stream); the buffers are validated as the parent validates them; no energy sample."""
    eng.step_wrench_tiled_sea(S, N, DT, 7.0, O, P6, STREAM)
    assert lib.calls == [("hydro_step_wrench_tiled_sea", (H, 1000, 0x10000000, 832, 0x20000000, 384, 0.01, 0x40000000, 384, 7.0, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.step_wrench_tiled_sea, O, N, DT, 1.0, out=O, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.step_wrench_tiled_sea, S, N, DT, 1.0, out=S, stream=STREAM)
    with_ke = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=STREAM, ke_out=KE)
    refused(lib, "the sea entry does not sample the kinetic energy (prepared with ke_out)", with_ke, 1.0)
    with_ke()
    assert lib.calls == [("hydro_step_wrench_tiled_ke", (H, 1000, 0x10000000, 832, 0x20000000, 384, 0.01, 0x40000000, 384, 1, 0x60000000, STREAM))]


@pytest.mark.parametrize("q", [False, True])
def test_step_wrench_aos_sea(lib, eng, q):
    head, out = (H, 1000, 0x70000000, 0x71000000, int(q), 0x72000000), (0x73000000, 0x74000000)
    sea = lambda dt, t: ("hydro_step_wrench_aos_sea", head + (dt,) + out + (t, STREAM))  # noqa: E731
    parent = lambda dt: ("hydro_step_wrench_aos", head + (dt,) + out + (STREAM,))  # noqa: E731
    assert eng.step_wrench_aos_sea(POS, ORI, VELS, DT, 3.25, F, TQ, quat_xyzw=q, stream=STREAM) == (F, TQ)
    assert lib.calls == [sea(0.01, 3.25)]
    lib.calls.clear()
    step = eng.prepare_step_wrench_aos(POS, ORI, VELS, F, TQ, quat_xyzw=q)
    assert lib.calls == []
    assert step(DT, STREAM) == (F, TQ) and step(DT, STREAM, None) == (F, TQ) and step(DT, STREAM, 0.0) == (F, TQ)
    assert step(0.02, stream=STREAM, time=0.01) == (F, TQ) and step(0.02, STREAM) == (F, TQ)
    assert lib.calls == [parent(0.01), parent(0.01), sea(0.01, 0.0), sea(0.02, 0.01), parent(0.02)]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (1000,6) tensor on cuda:0", eng.step_wrench_aos_sea, POS, ORI, T((N - 1, 6), 0x1000), DT, 1.0, F, TQ,
            stream=STREAM)


def test_sea_sample_at(lib, eng):
    """time 0 -> step index 0 (any dt > 0), time t -> (1, t): (double)1 * t == t exactly."""
    assert eng.sea_sample_at(S, N, 0.0, out=W, stream=STREAM) is W
    assert eng.sea_sample_at(S, N, 16666.666666666668, out=W, stream=STREAM) is W
    assert eng.sea_sample_at(S, N, 5e-324, out=W, stream=STREAM) is W
    (n0, a0), (n1, a1), (n2, a2) = lib.calls
    assert n0 == n1 == n2 == "hydro_sea_sample"
    assert a0[:5] == (H, 1000, 0x10000000, 832, 0) and a0[5] > 0.0 and a0[6:] == (0x98000000, 256, STREAM)
    assert a1 == (H, 1000, 0x10000000, 832, 1, 16666.666666666668, 0x98000000, 256, STREAM)
    assert a2[4:6] == (1, 5e-324)


# ---- the plugin, with a fake engine ----------------------------------------------------------------------------------------------
class FakeEngine:
    """Records what the plugin asks of an engine; nothing runs.  `built` lists the engines in the order they were made."""
    built: list = []

    def __init__(self, capacity, device, rho, g):
        self.device, self.n, self.calls = torch.device("cpu"), capacity, []
        FakeEngine.built.append(self)

    def set_params(self, rows):
        self.n = len(rows)

    def set_semantics(self, semantics):
        pass

    def sync(self):
        self.calls.append(("sync",))

    def set_sea(self, sea):
        self.calls.append(("set_sea", sea))

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
DTS = (1.0 / 60.0, 0.02, 1.0 / 90.0, 0.013)
MODES = pytest.mark.parametrize("batched", [True, "callbacks", False], ids=["scene", "callbacks", "per-prim"])


def _scene(batched, **kw):
    world, host, prims, behaviors = build_main_scene(batched=batched, device="cpu", **kw)
    for b in behaviors:
        b.on_play()
    return world, host, behaviors


def _steps(engine):
    return [c for c in engine.calls if c[0] == "step"]


def _sums(dts):
    """0, dt0, dt0 + dt1, ...: the fp64 sums in order."""
    out, t = [], 0.0
    for dt in dts:
        out.append(t)
        t = t + dt
    return out


@MODES
def test_without_a_sea_the_calls_are_todays(fake, batched):
    _, host, behaviors = _scene(batched)
    for dt in DTS[:3]:
        host.step(dt)
    assert len(fake.built) == (20 if batched is False else 1)
    for e in fake.built:
        assert e.calls == [("prepare",), ("step", DTS[0]), ("step", DTS[1]), ("step", DTS[2])]      # one positional argument: dt
    assert behaviors[0].sea_time == DTS[0] + DTS[1] + DTS[2]      # the clock runs all the same


@MODES
def test_with_a_sea_the_times_are_the_sums_of_the_earlier_deltas(fake, batched):
    _, host, behaviors = _scene(batched)
    hb.HydrodynamicsBehavior.set_sea(SEA)                        # before any engine exists
    for dt in DTS:
        host.step(dt)
    want = [("step", dt, None, t) for dt, t in zip(DTS, _sums(DTS))]
    assert want[0][3] == 0.0 and want[2][3] == DTS[0] + DTS[1]
    for e in fake.built:
        assert e.calls == [("prepare",), ("sync",), ("set_sea", SEA)] + want
    assert behaviors[3].sea_time == ((DTS[0] + DTS[1]) + DTS[2]) + DTS[3]


@MODES
def test_skipped_fetch_counts_and_the_guard_does_not(fake, batched):
    _, host, behaviors = _scene(batched)
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[0])
    for v in host.views:
        v.fail_next_fetch = True
    host.step(DTS[1])                                            # no step, but the callback counts
    host.step(1e-6)                                              # the reference's guard: not a callback at all
    host.step(0.0)
    host.step(DTS[2])
    for e in fake.built:
        assert _steps(e) == [("step", DTS[0], None, 0.0), ("step", DTS[2], None, DTS[0] + DTS[1])]


@MODES
def test_set_sea_reaches_engines_built_before_and_after_and_none_returns_to_the_parent(fake, batched):
    _, host, behaviors = _scene(batched)
    host.step(DTS[0])                                            # engines exist, no sea
    first = list(fake.built)
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[1])
    other = SeaState((0.0, 0.2, 0.0))
    behaviors[0].set_sea(other)                                  # may change between steps
    host.step(DTS[2])
    hb.HydrodynamicsBehavior.set_sea(None)
    host.step(DTS[3])
    host.step(DTS[0])
    t = _sums(DTS + DTS[:1])
    for e in first:
        assert e.calls == [("prepare",), ("step", DTS[0]), ("sync",), ("set_sea", SEA), ("step", DTS[1], None, t[1]),
                           ("sync",), ("set_sea", other), ("step", DTS[2], None, t[2]),
                           ("sync",), ("set_sea", None), ("step", DTS[3]), ("step", DTS[0])]
    # an engine built later (a prim leaves: the group rebuilds; per-prim: a behaviour stops and plays again) gets the sea too
    hb.HydrodynamicsBehavior.set_sea(SEA)
    behaviors[-1].on_stop()
    behaviors[-1].on_play()
    host.step(DTS[1])
    new = [e for e in fake.built if e not in first]
    assert len(new) == 1 and ("set_sea", SEA) in new[0].calls and _steps(new[0])[-1][:3] == ("step", DTS[1], None)


@pytest.mark.parametrize("batched", [True, "callbacks"], ids=["scene", "callbacks"])
def test_rebuild_keeps_the_clock_and_on_play_restarts_it(fake, batched):
    _, host, behaviors = _scene(batched)
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[0])
    host.step(DTS[1])
    behaviors[-1].on_stop()                                      # a membership change: the group rebuilds its engine at the next step
    host.step(DTS[2])
    assert len(fake.built) == 2
    assert _steps(fake.built[1]) == [("step", DTS[2], None, DTS[0] + DTS[1])]
    assert ("set_sea", SEA) in fake.built[1].calls
    # every prim stops: the group goes; played again, a new group starts a new clock
    for b in behaviors[:-1]:
        b.on_stop()
    for b in behaviors:
        b.on_play()
    host.step(DTS[3])
    assert _steps(fake.built[-1]) == [("step", DTS[3], None, 0.0)]


def test_a_per_prim_unit_restarts_its_clock_on_play(fake):
    _, host, behaviors = _scene(False)
    hb.HydrodynamicsBehavior.set_sea(SEA)
    host.step(DTS[0])
    host.step(DTS[1])
    behaviors[2].on_stop()
    behaviors[2].on_play()
    host.step(DTS[2])
    assert _steps(fake.built[-1]) == [("step", DTS[2], None, 0.0)]                    # units started at different moments:
    assert _steps(fake.built[0])[-1] == ("step", DTS[2], None, DTS[0] + DTS[1])       # different clocks


# ---- the JSON block ----------------------------------------------------------------------------------------------------------------
def _config(tmp_path, sea, gravity=9.81):
    data = cfg.default_config()
    data["globals"]["gravity"] = gravity
    if sea is not None:
        data["sea"] = sea
    path = os.path.join(tmp_path, cfg.CONFIG_FILE_NAME)
    json.dump(data, open(path, "w"))
    return path


def test_json_block_sets_the_sea(fake, tmp_path):
    assert "sea" not in cfg.default_config() and len(cfg.SCHEMA_NAMES) == 12
    block = {"current": [0.3, -0.1, 0.0], "waves": [{"height": 0.4, "period": 8.0, "heading_deg": 30.0, "phase": 0.25},
                                                     {"height": 0.1, "period": 3.0, "heading_deg": -80.0, "phase": 0.0}]}
    path = _config(tmp_path, block, gravity=9.8)
    build_main_scene(config_path=path, device="cpu")
    sea = hb.REGISTRY.sea
    assert sea is not None and sea.current == (0.3, -0.1, 0.0) and len(sea.waves) == 2
    for got, w in zip(sea.waves, block["waves"]):
        want, = SeaState.regular(w["height"], w["period"], w["heading_deg"], w["phase"], g=9.8).waves     # the FILE's gravity
        assert all(abs(a - b) <= 1e-12 for a, b in zip(got, want))
    not_this, = SeaState.regular(0.4, 8.0, 30.0, 0.25, g=9.81).waves
    assert abs(sea.waves[0][1] - not_this[1]) > 1e-6
    # the attributes still come from the same file
    assert cfg.resolve_overrides("Body", json.load(open(path)))["gravity"] == 9.8


@pytest.mark.parametrize("block", [{"current": [0.1, 0.2]}, {"waves": [{"height": 0.4}]}, {"waves": [{"height": 0.4, "period": -1.0}]}, [1, 2, 3],
                                   {"current": [0.0, 0.0, 0.0], "swell": 1}, {"waves": [{"height": 0.2, "period": 4.0}] * 9}, {"current": [0.0, "x", 0.0]}])
def test_a_malformed_block_is_logged_and_ignored(fake, tmp_path, caplog, block):
    path = _config(tmp_path, block)
    with caplog.at_level(logging.ERROR, logger="silver2_isaacsim_amd"):
        _, host, prims, _ = build_main_scene(config_path=path, device="cpu")
    assert hb.REGISTRY.sea is None and hb.REGISTRY._sea_source is None
    assert any("[Hydro] JSON Error" in r.getMessage() for r in caplog.records)
    # the rest of the file was applied
    body = next(p for p in prims if p.GetName() == "Body")
    assert host.get_exposed_variable(body, cfg.full_attr_name("liftCoefficient")) == 0.5


def test_a_sea_set_from_python_wins_and_only_the_first_block_counts(fake, tmp_path):
    mine = SeaState((0.0, 0.5, 0.0))
    hb.HydrodynamicsBehavior.set_sea(mine)
    build_main_scene(config_path=_config(tmp_path, {"current": [1.0, 0.0, 0.0]}), device="cpu")
    assert hb.REGISTRY.sea is mine
    hb.REGISTRY.clear()
    build_main_scene(config_path=_config(tmp_path, {"current": [1.0, 0.0, 0.0]}), device="cpu")
    first = hb.REGISTRY.sea
    assert first.current == (1.0, 0.0, 0.0)
    build_main_scene(config_path=_config(tmp_path, {"current": [2.0, 0.0, 0.0]}), device="cpu")
    assert hb.REGISTRY.sea is first
    # a file without the block sets nothing
    hb.REGISTRY.clear()
    build_main_scene(config_path=_config(tmp_path, None), device="cpu")
    assert hb.REGISTRY.sea is None and hb.REGISTRY._sea_source is None
