"""The sea state (hydro_set_sea, hydro_sea_sample, hydro_step_fused_tiled_multi_sea; silver2_isaacsim_amd.sea.SeaState) as far
as a machine without a GPU can see it: the dispersion relation of SeaState.regular, the host restatement against the fp64
reference of tests/sea_reference.py, the C boundary, the Python host's marshalling (with the stand-ins of
tests/test_engine_calls.py), ClosedLoopSim's bookkeeping with a fake engine, and the two physical checks the device tests lean
on, run through closed_loop_reference.closed_loop."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sea_reference as sr
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd.sea import SeaState
from designed_populations import drift_scene, _test_sea, wave_scene
from engine_stand_ins import eng, FUSED_HEAD, H, KE, lib, N, P13, refused, S, SO, STREAM, T, TILES  # noqa: F401  (fixtures are requested by name)

ENTRIES = ("hydro_set_sea", "hydro_sea_sample", "hydro_step_fused_tiled_multi_sea")
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
W = T((TILES, 4, 64), 0x98000000)                                 # the sample's output


# ---- SeaState ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heading", [0.0, 30.0, 90.0, 200.0, -45.0])
def test_regular_obeys_the_deep_water_dispersion_relation(heading):
    for height, period, g in ((0.4, 8.0, 9.81), (1.5, 3.0, 9.81), (0.1, 12.0, 1.62)):
        sea = SeaState.regular(height, period, heading, phase=0.25, g=g)
        (a, kx, ky, om, ph), = sea.waves
        kappa = math.hypot(kx, ky)
        assert a == 0.5 * height and ph == 0.25 and om == pytest.approx(2.0 * math.pi / period, rel=1e-15)
        assert om * om == pytest.approx(g * kappa, rel=1e-14)
        assert kx == pytest.approx(kappa * math.cos(math.radians(heading)), abs=1e-15 * kappa)
        assert ky == pytest.approx(kappa * math.sin(math.radians(heading)), abs=1e-15 * kappa)
        assert sea.current == (0.0, 0.0, 0.0)


def test_sea_state_refuses_what_the_library_refuses():
    sea = SeaState((0.1, 0.2, 0.0))
    for bad in ((-0.1, 1.0, 0.0, 1.0, 0.0), (0.1, 0.0, 0.0, 1.0, 0.0), (float("nan"), 1.0, 0.0, 1.0, 0.0), (0.1, float("inf"), 0.0, 1.0, 0.0)):
        with pytest.raises(ValueError):
            sea.add_wave(*bad)
    with pytest.raises(ValueError):
        SeaState((0.0, float("nan"), 0.0))
    for _ in range(8):
        sea.add_wave(0.1, 0.5, 0.0, 2.0)
    with pytest.raises(ValueError, match="at most 8"):
        sea.add_wave(0.1, 0.5, 0.0, 2.0)
    assert len(sea.waves) == 8 and SeaState().add_wave(0.0, 0.0, 0.0, 0.0).waves == [(0.0, 0.0, 0.0, 0.0, 0.0)]


def test_host_restatement_equals_the_reference():
    sea = _test_sea()
    rng = np.random.default_rng(5)
    x, y, z = rng.uniform(-200, 200, 500), rng.uniform(-200, 200, 500), rng.uniform(-30, 2, 500)
    for step in (0, 1, 7, 10 ** 6):
        t = step / 60.0
        eta, u = sr.water(sea, x, y, z + sea.elevation(x, y, t), step, 1.0 / 60.0)
        assert np.abs(sea.elevation(x, y, t) - eta).max() <= 1e-12
        assert np.abs(sea.velocity(x, y, z, t) - u).max() <= 1e-12
    # by hand: one wave along +x at its crest, at the surface and one e-folding depth below it
    one = SeaState((0.1, 0.0, 0.0)).add_wave(0.5, 0.2, 0.0, 1.4, 0.0)
    assert one.elevation(0.0, 3.0, 0.0) == 0.5
    assert np.allclose(one.velocity(0.0, 0.0, [0.0, 1.0, -5.0], 0.0), [[0.8, 0, 0], [0.8, 0, 0], [0.1 + 0.7 / math.e, 0, 0]], rtol=1e-15, atol=0)
    # a quarter period later the crest has passed: the surface goes through zero and the water moves down, u_z = a omega sin th
    quarter = 0.5 * math.pi / 1.4
    assert abs(one.elevation(0.0, 0.0, quarter)) < 1e-16 and one.velocity(0.0, 0.0, 0.0, quarter)[2] == pytest.approx(-0.7, rel=1e-15)


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert int(re.search(r"#define HYDRO_SEA_WAVES_MAX\s+(\d+)", code).group(1)) == nat.SEA_WAVES_MAX == 8
    assert int(re.search(r"#define HYDRO_SEA_FIELDS\s+(\d+)", code).group(1)) == nat.SEA_FIELDS == 4
    # the pose-hold entry's argument list with step0 in front of the stream
    ctl, sea = nat.SIGNATURES["hydro_step_fused_tiled_multi_ctl"], nat.SIGNATURES["hydro_step_fused_tiled_multi_sea"]
    assert sea[0] is ctl[0] and sea[1] == ctl[1][:-1] + [ctypes.c_int64] + ctl[1][-1:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto("hydro_step_fused_tiled_multi_sea") == proto("hydro_step_fused_tiled_multi_ctl").replace(
        ", void *stream", ", int64_t step0, void *stream")
    # hydro_sea_t as ctypes lays it out is what the C compiler lays out: 3 doubles, an int (padded), 8 x 5 doubles
    assert ctypes.sizeof(nat.SeaWave) == 40 and ctypes.sizeof(nat.Sea) == 24 + 8 + 8 * 40 and nat.Sea.wave.offset == 32
    # every limit of the model is stated
    for phrase in ("slope of the surface", "long-wave approximation", "Froude-Krylov", "added-mass term", "finite depth", "not volume-conserving"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_sea(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                               None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_set_sea(None, None) == -1 and lib_.hydro_set_sea(None, ctypes.byref(nat.Sea())) == -1
    assert lib_.hydro_sea_sample(None, 64, None, 832, 0, 1 / 60, None, 256, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_set_sea_marshals_the_struct(lib, eng):
    sea = SeaState((0.5, -0.2, 0.05)).add_wave(0.2, 0.06, 0.02, 0.8, 0.3).add_wave(0.1, -0.1, 0.2, 1.5)
    eng.set_sea(sea)
    zero = (0.0,) * 5
    assert lib.calls == [("hydro_set_sea", (H, ("byref", ((0.5, -0.2, 0.05), 2, ((0.2, 0.06, 0.02, 0.8, 0.3), (0.1, -0.1, 0.2, 1.5, 0.0)) + (zero,) * 6))))]
    assert eng.sea_waves == 2
    lib.calls.clear()
    eng.set_sea(SeaState((0.1, 0.0, 0.0)))
    assert lib.calls == [("hydro_set_sea", (H, ("byref", ((0.1, 0.0, 0.0), 0, (zero,) * 8))))] and eng.sea_waves == 0
    lib.calls.clear()
    eng.set_sea(None)
    assert lib.calls == [("hydro_set_sea", (H, None))] and eng.sea_waves is None

    class Nine:
        current, waves = (0.0, 0.0, 0.0), [(0.1, 1.0, 0.0, 1.0, 0.0)] * 9
    lib.calls.clear()
    refused(lib, "a sea has at most 8 wave components of (amplitude, kx, ky, omega, phase)", eng.set_sea, Nine())


def test_sea_sample(lib, eng):
    assert eng.sea_sample(S, N, 10 ** 6, 0.01, out=W, stream=STREAM) is W
    assert lib.calls == [("hydro_sea_sample", (H, 1000, 0x10000000, 832, 10 ** 6, 0.01, 0x98000000, 256, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 4, 64) tensor on cuda:0", eng.sea_sample, S, N, 0, 0.01, out=A, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.sea_sample, A, N, 0, 0.01, out=W, stream=STREAM)


def test_step_fused_tiled_multi_sea(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    cases = [(dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0, 0, STREAM)),
             (dict(control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088, 123456789012, STREAM)),
             (dict(applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0, 5, STREAM))]
    for kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_sea(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [("hydro_step_fused_tiled_multi_sea", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_sea, S, P13, N, 0.01, 3, 0, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 17, 64) tensor on cuda:0", eng.step_fused_tiled_multi_sea, S, P13, N, 0.01, 3, 0, A, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class FakeEngine:
    """Records the stepping calls ClosedLoopSim makes; nothing runs."""

    def __init__(self):
        self.calls = []

    def set_sea(self, sea):
        self.calls.append(("set_sea", sea))

    def step_fused_tiled_multi_sea(self, cur, old, n, dt, steps, step0, control, applied, frame, **kw):
        self.calls.append(("sea", steps, step0, control, applied, cur))
        return 0

    def step_fused_tiled_multi(self, cur, old, n, dt, steps, **kw):
        self.calls.append(("plain", steps))

    def step_fused_tiled(self, cur, old, n, dt, **kw):
        self.calls.append(("single",))


class _Ctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.fixture
def sim(monkeypatch):
    monkeypatch.setattr(simulate.torch.cuda, "stream", lambda s: _Ctx())
    s = object.__new__(simulate.ClosedLoopSim)
    s.fused, s.implicit_drag, s.n, s.dt, s.engine = True, False, 64, 1.0 / 60.0, FakeEngine()
    s.cur, s.old, s.stream = "buffer A", "buffer B", None
    s.steps_done, s.monitor, s._monitor_warm, s.recorder = 0, None, True, None
    s.applied, s.applied_frame, s.control, s.sea = None, "body", None, None
    s._graph, s._graph_steps, s._graph_bufs = None, 0, None
    s.synchronize = lambda timeout_s=None: None
    return s


def test_step0_follows_steps_done(sim):
    waves = SeaState.regular(0.4, 8.0, 0.0)
    sim.run_resident(3, chunk=2)
    assert sim.engine.calls == [("plain", 2), ("plain", 1)]
    sim.engine.calls.clear()
    sim.set_sea(waves)
    assert sim.engine.calls == [("set_sea", waves)] and sim.sea is waves
    sim.engine.calls.clear()
    sim.run_eager(2)
    sim.run_resident(130, chunk=64)
    sim.run(3, graph_steps=0)                                    # no replays asked for: eager steps
    assert [c[:3] for c in sim.engine.calls] == [("sea", 1, 3), ("sea", 1, 4), ("sea", 64, 5), ("sea", 64, 69), ("sea", 2, 133),
                                                 ("sea", 1, 135), ("sea", 1, 136), ("sea", 1, 137)]
    assert [c[5] for c in sim.engine.calls[:4]] == ["buffer A", "buffer B", "buffer A", "buffer B"]     # the ping-pong goes on
    assert sim.steps_done == 138
    sim.engine.calls.clear()
    sim.control = "hold"
    sim.run_resident(2, chunk=2)
    assert sim.engine.calls == [("sea", 2, 138, "hold", None, sim.old)]
    sim.engine.calls.clear()
    sim.control = None
    sim.clear_sea()
    sim.run_resident(2, chunk=2)
    assert sim.engine.calls == [("set_sea", None), ("plain", 2)] and sim.sea is None


def test_graph_replays_refuse_waves_and_take_a_current(sim, monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    sim.set_sea(SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0)))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        sim.run(64, graph_steps=32)
    assert captured == [] and sim.steps_done == 0
    sim.run(3, graph_steps=32)                                   # fewer steps than a replay: eager, legal
    assert sim.steps_done == 3
    sim.set_sea(SeaState((0.3, 0.0, 0.0)))
    sim._graph = "a captured graph of the other sea"
    sim.set_sea(SeaState((0.4, 0.0, 0.0)))
    assert sim._graph is None                                    # captured launches are of another sea's entry
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        sim.run(64, graph_steps=32)
    assert captured == [32]


def test_set_sea_needs_the_fused_step(sim):
    sim.fused = False
    with pytest.raises(ValueError, match="fused"):
        sim.set_sea(SeaState((0.1, 0.0, 0.0)))
    assert sim.sea is None and sim.engine.calls == []


# ---- the physics the device tests lean on ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_a_body_released_into_a_current_drifts_with_it(implicit):
    st, pv, pr, sea = drift_scene()
    run = closed_loop(st, pv, pr, scenes.RHO, scenes.G, float(np.float32(1.0 / 60.0)), 1200, sea=sea, implicit=implicit)
    v, U = run[-1]["state"][0, 7:10].astype(np.float64), np.asarray(sea.current)
    drift = np.linalg.norm(v - U) / np.linalg.norm(U)
    print(f"[drift, {'implicit' if implicit else 'explicit'}] |v - U| / |U| after 1 200 steps: {drift:.3e}")
    assert drift < 1e-2
    assert abs(float(run[-1]["state"][0, 2]) + 10.0) < 1e-3       # and stays at its depth


def test_a_buoy_rides_the_wave():
    sc, sea, z_eq = wave_scene()
    run = closed_loop(sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt, 1920, sea=sea, implicit=False)
    dev = np.array([abs(float(r["state"][0, 2]) - z_eq - float(sea.elevation(r["state"][0, 0], r["state"][0, 1], (k + 1) * sc.dt)))
                    for k, r in enumerate(run)])
    print(f"[wave] largest |z - z_eq - eta| after step 480: {dev[480:].max():.4f} m (over the whole run {dev.max():.4f} m)")
    assert dev[480:].max() < 0.1
