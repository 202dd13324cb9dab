"""The seabed (hydro_set_seabed, hydro_seabed_wrench, hydro_step_fused_tiled_multi_bed; silver2_isaacsim_amd.seabed.Seabed) as
far as a machine without a GPU can see it: the C boundary, the Python host's marshalling (with the stand-ins of
tests/test_engine_calls.py), ClosedLoopSim's bookkeeping with a fake engine, the host restatement against the fp64 reference
of tests/seabed_reference.py and cases worked by hand, and the physics - boxes that sink, land and come to rest, and a resting
box that is pushed - through closed_loop_reference.closed_loop.  (hydro_set_seabed's own refusals need an engine, hence a
device: tests/test_seabed_gpu.py; the refusals of the Seabed dataclass, which are the same list, are here.)

THE PUSHED BOX.  The friction of the model is capped at the damping m gamma per corner, so below the Coulomb limit a resting
box does not stick: it creeps at F / (4 m gamma).  For the 0.5 m cube at twice the water's density pushed with
0.5 mu N_total that is 0.128 m/s at dt = 1/60 (gamma = 2.4 / s) and 0.064 m/s at 1/120; measured on the reference, 5 s of push
move it 0.584 m and 0.311 m (the water's drag takes the rest).  The bound is twice the measured creep.  With 2 mu N_total the
friction saturates at mu N and the box runs away: 5.80 m in 5 s at either step."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import seabed_reference as br
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from designed_populations import BOXES, PENETRATION, rest_report, REST_V, REST_W, REST_Z, settling_boxes, Z_B
from engine_stand_ins import eng, FUSED_HEAD, H, KE, lib, N, P13, refused, S, SO, STREAM, T, TILES  # noqa: F401  (fixtures are requested by name)

ENTRIES = ("hydro_set_seabed", "hydro_seabed_wrench", "hydro_step_fused_tiled_multi_bed")
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
W = T((TILES, 6, 64), 0x98000000)                                 # the probe's output
BED = Seabed(-5.0, 144.0, 2.4, 0.5, 0.01, 2.4)


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    # exactly the sea entry's argument list
    assert nat.SIGNATURES["hydro_step_fused_tiled_multi_bed"] == nat.SIGNATURES["hydro_step_fused_tiled_multi_sea"]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto("hydro_step_fused_tiled_multi_bed") == proto("hydro_step_fused_tiled_multi_sea")
    # hydro_seabed_t: six doubles, in the order of the table
    body = re.search(r"typedef struct hydro_seabed \{(.*?)\} hydro_seabed_t;", code, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "double z, stiffness, damping, friction, slip_speed, friction_rate;"
    assert [f for f, _ in nat.Seabed._fields_] == ["z", "stiffness", "damping", "friction", "slip_speed", "friction_rate"]
    assert ctypes.sizeof(nat.Seabed) == 48 and all(t is ctypes.c_double for _, t in nat.Seabed._fields_)
    # the header says what the bed does not see, what is not modelled, and which entries ignore it
    for phrase in ("THE SEA DOES NOT TOUCH THE BED", "never the state relative to the water", "deep-water one", "slope and terrain",
                   "rolling and spinning friction", "face or edge contact other than through the corners", "body-to-body contact",
                   "the other five closed-loop entries", "kappa dt^2 <= 0.04", "beta dt, gamma dt <= 0.04"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_bed(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                               None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_set_seabed(None, None) == -1 and lib_.hydro_set_seabed(None, ctypes.byref(nat.Seabed(-5, 144, 2.4, 0.5, 0.01, 2.4))) == -1
    assert lib_.hydro_seabed_wrench(None, 64, None, 832, None, 384, None) == -1


def test_the_dataclass_refuses_what_the_library_refuses():
    nan, inf = float("nan"), float("inf")
    good = dict(z=-5.0, stiffness=144.0, damping=2.4, friction=0.5, slip_speed=0.01, friction_rate=2.4)
    Seabed(**good)
    Seabed(**{**good, "z": 3.0, "stiffness": 0.0, "damping": 0.0, "friction": 0.0, "friction_rate": 0.0})     # every edge that is legal
    for key in good:
        for bad in (nan, inf, -inf):
            with pytest.raises(ValueError):
                Seabed(**{**good, key: bad})
    for key in ("stiffness", "damping", "friction", "friction_rate"):
        with pytest.raises(ValueError, match=">= 0"):
            Seabed(**{**good, key: -1e-9})
    for bad in (0.0, -0.01):
        with pytest.raises(ValueError, match="slip_speed"):
            Seabed(**{**good, "slip_speed": bad})


def test_for_step_gives_the_documented_defaults():
    for dt in (1 / 60, 1 / 120, 1 / 240):
        bed = Seabed.for_step(-5.0, dt)
        assert bed.z == -5.0 and bed.friction == 0.5 and bed.slip_speed == 0.01
        assert bed.stiffness * dt * dt == pytest.approx(0.04, rel=1e-14) and bed.damping * dt == pytest.approx(0.04, rel=1e-14)
        assert bed.friction_rate == bed.damping
        assert bed.rest_depth(2.0, 9.81) == pytest.approx(9.81 * 0.5 / (4 * bed.stiffness), rel=1e-15)
    assert Seabed.for_step(2.0, 0.01, friction=0.8, slip_speed=0.02) == Seabed(2.0, 400.0, 4.0, 0.8, 0.02, 4.0)
    with pytest.raises(ValueError):
        Seabed.for_step(-5.0, 0.0)


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_set_seabed_marshals_the_struct(lib, eng):
    eng.set_seabed(BED)
    assert lib.calls == [("hydro_set_seabed", (H, ("byref", (-5.0, 144.0, 2.4, 0.5, 0.01, 2.4))))] and eng.seabed is BED
    lib.calls.clear()
    eng.set_seabed(None)
    assert lib.calls == [("hydro_set_seabed", (H, None))] and eng.seabed is None


def test_seabed_wrench(lib, eng):
    assert eng.seabed_wrench(S, N, out=W, stream=STREAM) is W
    assert lib.calls == [("hydro_seabed_wrench", (H, 1000, 0x10000000, 832, 0x98000000, 384, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.seabed_wrench, S, N, out=C, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.seabed_wrench, A, N, out=W, stream=STREAM)


def test_step_fused_tiled_multi_bed(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    cases = [(dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0, 0, STREAM)),
             (dict(control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088, 123456789012, STREAM)),
             (dict(applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0, 5, STREAM))]
    for kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_bed(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [("hydro_step_fused_tiled_multi_bed", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_bed, S, P13, N, 0.01, 3, 0, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 17, 64) tensor on cuda:0", eng.step_fused_tiled_multi_bed, S, P13, N, 0.01, 3, 0, A, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class FakeEngine:
    """Records the calls ClosedLoopSim makes; nothing runs."""

    def __init__(self):
        self.calls = []

    def set_seabed(self, bed):
        self.calls.append(("set_seabed", bed))

    def set_sea(self, sea):
        self.calls.append(("set_sea", sea))

    def _step(self, name, cur, steps, **kw):
        self.calls.append(dict(method=name, cur=cur, steps=steps, **kw))
        return 0

    def step_fused_tiled_multi_bed(self, cur, old, n, dt, steps, step0, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("bed", cur, steps, step0=step0, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_sea(self, cur, old, n, dt, steps, step0, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("sea", cur, steps, step0=step0, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_controlled(self, cur, old, n, dt, steps, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("ctl", cur, steps, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_applied(self, cur, old, n, dt, steps, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("app", cur, steps, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_rec(self, cur, old, n, dt, steps, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("rec", cur, steps, log=log)

    def step_fused_tiled_multi(self, cur, old, n, dt, steps, **kw):
        self._step("plain", cur, steps)

    def step_fused_tiled(self, cur, old, n, dt, **kw):
        self._step("single", cur, None)


class _Ctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _sim(monkeypatch, recorder=False, applied=False, control=False, sea=False):
    monkeypatch.setattr(simulate.torch.cuda, "stream", lambda s: _Ctx())
    s = object.__new__(simulate.ClosedLoopSim)
    s.fused, s.implicit_drag, s.n, s.dt, s.engine = True, True, 64, 1.0 / 60.0, FakeEngine()
    s.cur, s.old, s.stream = "buffer A", "buffer B", None
    s.steps_done, s.monitor, s._monitor_warm, s.ke_dev = 0, None, True, None
    s.recorder = simulate.TrajectoryRecorder([5, 2], every=2, rows=64, sim=s) if recorder else None
    s.applied, s.applied_frame = ("the applied buffer" if applied else None), "world"
    s.control = "the control buffer" if control else None
    s.sea = SeaState((0.3, 0.0, 0.0)) if sea else None
    s._graph, s._graph_steps, s._graph_bufs = None, 0, None
    s.synchronize = lambda timeout_s=None: None
    return s


# what the sim calls without a bed, by the rule of tests/test_sim_dispatch.py
def _without_bed(recorder, applied, control, sea, eager):
    return "sea" if sea else "ctl" if control else "app" if applied else "rec" if recorder else "single" if eager else "plain"


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=4)),
                         ids=lambda c: "".join(n for n, on in zip(("rec", "App", "Ctl", "Sea"), c) if on) or "plain")
def test_the_bed_entry_is_picked_with_every_combination_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, sea = combo
    s = _sim(monkeypatch, *combo)
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    s.set_seabed(BED)
    assert s.engine.calls == [("set_seabed", BED)] and s.seabed is BED
    s.engine.calls.clear()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "bed" and call["steps"] == k and call["step0"] == done
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer A", "buffer B")[i % 2]
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_seabed()
    assert s.engine.calls == [("set_seabed", None)] and s.seabed is None
    s.engine.calls.clear()
    go()
    want = _without_bed(recorder, applied, control, sea, eager=run != "resident")
    assert [c["method"] for c in s.engine.calls] == [want] * 3
    s.clear_seabed()                                             # a second clear is nothing
    assert len(s.engine.calls) == 3


def test_graph_replays_take_a_bed_and_a_current_and_refuse_waves(monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s = _sim(monkeypatch)
    s._graph = "a captured graph without a bed"
    s.set_seabed(BED)
    assert s._graph is None                                      # captured launches are of another entry
    s.sea = SeaState((0.3, 0.0, 0.0))
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]
    s.sea = SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [32] and s.steps_done == 0
    s._graph = "a captured graph with the bed"
    s.clear_seabed()
    assert s._graph is None


def test_set_seabed_needs_the_fused_step(monkeypatch):
    s = _sim(monkeypatch)
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_seabed(BED)
    assert s.seabed is None and s.engine.calls == []


# ---- the host restatement ------------------------------------------------------------------------------------------------------------
def _random_bodies(n, seed, z_b):
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 13))
    st[:, 0:2] = rng.uniform(-50, 50, (n, 2))
    st[:, 2] = z_b + rng.uniform(-0.3, 0.8, n)
    q = rng.normal(size=(n, 4))
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))          # non-unit included
    st[:, 7:13] = rng.uniform(-1, 1, (n, 6))
    pr = np.zeros((n, 11))
    pr[:, 0:3] = rng.uniform(0.1, 1.2, (n, 3))
    pr[:, 3:10] = scenes._DEFAULT_COEFFS
    pr[:, 10] = rng.uniform(1.05, 8.0, n) * scenes.RHO * pr[:, 0:3].prod(axis=1)
    return st, pr


def test_host_restatement_equals_the_reference():
    st, pr = _random_bodies(600, 11, BED.z)
    count = br.corner_count(BED, st, pr)
    assert (count == 0).sum() > 50 and ((count > 0) & (count < 4)).sum() > 50 and (count >= 4).sum() > 50
    ref, got = br.wrench(BED, st, pr), BED.wrench(st, pr)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(ref).max() > 100.0
    assert not got[count == 0].any() and (got[count > 0, 2] >= 0).all()
    assert np.abs(BED.corners(st, pr) - br.corners(st, pr)).max() <= 1e-15


def test_the_header_s_fp32_order_stands_within_the_probe_bound_of_fp64():
    """The operations include/hydro.h lists, carried out in NumPy float32 (seabed_reference.wrench_fp32_emulated), against the
    fp64 reference with the same corners contributing, in units of 2^-24 of seabed_reference.wrench_scales: what the stated
    order costs before any hardware is involved.  1.80 (force) and 0.61 (torque) here; the bound is the device test's, 4."""
    st, pr = (a.astype(np.float32) for a in _random_bodies(600, 11, BED.z))
    touch = br.touching_fp32(BED, st, pr)
    got, ref, scale = br.wrench_fp32_emulated(BED, st, pr), br.wrench(BED, st, pr, touch), br.wrench_scales(BED, st, pr, touch)
    on = touch.any(axis=1)
    assert not got[~on].any() and on.sum() > 300
    err = np.abs(got[on] - ref[on]) / (br.ULP * np.where(scale == 0, 1.0, scale)[on])
    print(f"[seabed, fp32 order emulated on the host] force {err[:, 0:3].max():.2f}  torque {err[:, 3:6].max():.2f} units of 2^-24 of the scale")
    assert err.max() <= 4.0


def test_one_corner_by_hand():
    """A unit cube of 20 kg balanced on one corner - its body diagonal (-1, -1, -1) turned onto -z - with that corner 1 cm below
    the plane (the next three are 0.58 m higher), sliding and sinking without spin: one spring, one damper, one friction force
    at r = (0, 0, -sqrt(3) / 2).  Then the same corner leaving the bed (no adhesion), and the cap."""
    # one corner: the cube diagonal pointing down.  Unit cube 1 m, the body frame's (-1, -1, -1) direction turned onto -z.
    d = np.array([-1.0, -1.0, -1.0]) / np.sqrt(3.0)
    axis = np.cross(d, [0.0, 0.0, -1.0])
    s_, c_ = np.linalg.norm(axis), float(d @ [0.0, 0.0, -1.0])
    ang = np.arctan2(s_, c_)
    q = np.concatenate([axis / s_ * np.sin(ang / 2), [np.cos(ang / 2)]])
    half_diag = np.sqrt(3.0) / 2.0
    bed = Seabed(z=-2.0, stiffness=100.0, damping=3.0, friction=0.5, slip_speed=0.05, friction_rate=1000.0)
    m, depth = 20.0, 0.01
    st = np.zeros((1, 13))
    st[0, 2] = -2.0 + half_diag - depth                          # the lowest corner 1 cm below the plane; the next ones are 0.58 m higher
    st[0, 3:7] = q
    st[0, 7:10] = (0.12, -0.05, -0.2)                            # sliding along +x and -y, sinking at 0.2 m/s; no spin
    pr = np.zeros((1, 11))
    pr[0, 0:3], pr[0, 10] = 1.0, m
    assert br.corner_count(bed, st, pr)[0] == 1
    N = m * (100.0 * depth - 3.0 * -0.2)                         # 20 (1 + 0.6) = 32 N
    c = 0.5 * N / np.sqrt(0.12 ** 2 + 0.05 ** 2 + 0.05 ** 2)     # far below the cap of 20 000
    F = np.array([-c * 0.12, c * 0.05, N])
    r = np.array([0.0, 0.0, -half_diag])
    want = np.concatenate([F, np.cross(r, F)])
    assert N == pytest.approx(32.0, rel=1e-12)
    for got in (bed.wrench(st, pr)[0], br.wrench(bed, st, pr)[0]):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # no adhesion: leaving the bed faster than the spring pushes gives no force at all, though the corner is still below
    st[0, 9] = 0.5
    assert not bed.wrench(st, pr).any() and br.corner_count(bed, st, pr)[0] == 1
    # the cap: friction_rate 0.1 / s limits c to m gamma = 2
    st[0, 9] = -0.2
    capped = Seabed(-2.0, 100.0, 3.0, 0.5, 0.05, 0.1).wrench(st, pr)[0]
    assert capped[:3] == pytest.approx([-2.0 * 0.12, 2.0 * 0.05, 32.0], rel=1e-12)


def test_four_corners_by_hand():
    """A 0.4 x 0.2 x 0.1 m box of 10 kg lying flat, its bottom 2 mm below the plane, sliding along +x at 0.3 m/s and spinning
    about z at 0.5 rad/s: N is the same at the four lower corners, the friction follows each corner's own velocity, and the
    wrench has no roll or pitch torque from N (the corners are symmetric)."""
    bed = Seabed(z=-3.0, stiffness=200.0, damping=0.0, friction=0.4, slip_speed=0.01, friction_rate=1e6)
    m = 10.0
    st = np.zeros((1, 13))
    st[0, 2], st[0, 6], st[0, 7], st[0, 12] = -3.0 + 0.05 - 0.002, 1.0, 0.3, 0.5
    pr = np.zeros((1, 11))
    pr[0, 0:3], pr[0, 10] = (0.4, 0.2, 0.1), m
    assert br.corner_count(bed, st, pr)[0] == 4
    N = m * 200.0 * 0.002                                        # 4 N per corner
    F_tot, T_tot = np.zeros(3), np.zeros(3)
    for sx in (-1, 1):
        for sy in (-1, 1):
            r = np.array([sx * 0.2, sy * 0.1, -0.05])
            u = np.array([0.3 - 0.5 * r[1], 0.5 * r[0], 0.0])    # v + omega x r with omega = (0, 0, 0.5)
            c = 0.4 * N / np.sqrt(u[0] ** 2 + u[1] ** 2 + 1e-4)
            F = np.array([-c * u[0], -c * u[1], N])
            F_tot += F
            T_tot += np.cross(r, F)
    want = np.concatenate([F_tot, T_tot])
    assert want[2] == pytest.approx(16.0, rel=1e-12) and want[0] < 0 and abs(want[1]) < 1e-12      # it brakes the slide; F_y cancels in pairs
    assert abs(want[3]) < 1e-12 and want[4] == pytest.approx(-0.05 * want[0], rel=1e-12)             # N gives no roll; the friction pitches
    for got in (bed.wrench(st, pr)[0], br.wrench(bed, st, pr)[0]):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- the physics: boxes that sink, land and rest --------------------------------------------------------------------------------------


@pytest.mark.parametrize("rate", [60, 120])
def test_boxes_sink_land_and_come_to_rest(rate):
    st, pv, pr, ratios = settling_boxes()
    dt = float(np.float32(1.0 / rate))
    bed = Seabed.for_step(Z_B, dt)
    run = closed_loop(st, pv, pr, scenes.RHO, scenes.G, dt, 12 * rate, bed=bed, implicit=True)
    deepest = np.max([r["delta"].max(axis=1) for r in run], axis=0)
    contacts, v, w, off = rest_report(bed, run[-1]["state"], pr, ratios)
    print(f"[rest, dt = 1/{rate}] corners {contacts.tolist()}  |v| <= {v.max():.2e} m/s  |omega| <= {w.max():.2e} rad/s  "
          f"lowest corner off the analytic depth by <= {off.max():.2e} m  deepest transient {deepest.max():.3f} m (box {int(deepest.argmax())})")
    assert (contacts == 4).all(), contacts
    assert v.max() < REST_V and w.max() < REST_W, (v, w)
    assert off.max() < REST_Z, off
    assert deepest.max() < PENETRATION, deepest
    assert deepest.max() > 0.01                                  # and they did land


def pushed_box(rate):
    """The 0.5 m cube at twice the water's density at rest on the bed; N_total, its weight in water."""
    dims, ratio = BOXES[0]
    dt = float(np.float32(1.0 / rate))
    bed = Seabed.for_step(Z_B, dt)
    m = ratio * scenes.RHO * np.prod(dims)
    st = np.zeros((1, 13), np.float32)
    st[0, 2], st[0, 6] = Z_B + 0.25 - bed.rest_depth(ratio, scenes.G), 1.0
    pr = np.concatenate([dims, scenes._DEFAULT_COEFFS, [m]])[None, :].astype(np.float32)
    return st, pr, bed, dt, m * scenes.G * (1.0 - 1.0 / ratio)


CREEP = {60: 0.584, 120: 0.311}                                   # m in 5 s under 0.5 mu N_total, measured on the reference (module docstring)


@pytest.mark.parametrize("rate", [60, 120])
def test_a_resting_box_creeps_under_half_the_friction_limit_and_runs_away_over_twice_it(rate):
    st, pr, bed, dt, n_total = pushed_box(rate)
    moved = {}
    for factor in (0.5, 2.0):
        push = np.zeros((1, 6))
        push[0, 0] = factor * bed.friction * n_total
        run = closed_loop(st, np.zeros((1, 6), np.float32), pr, scenes.RHO, scenes.G, dt, 5 * rate, bed=bed, implicit=True, applied=push)
        moved[factor] = float(run[-1]["state"][0, 0])
        assert abs(float(run[-1]["state"][0, 2]) - float(st[0, 2])) < 1e-3          # it stays on the bed
    creep_speed = 0.5 * bed.friction * n_total / (4.0 * float(pr[0, 10]) * bed.friction_rate)
    print(f"[push, dt = 1/{rate}] 0.5 mu N: {moved[0.5]:.3f} m in 5 s (creep speed F / (4 m gamma) = {creep_speed:.3f} m/s)   2 mu N: {moved[2.0]:.2f} m")
    assert 0.0 < moved[0.5] < 2.0 * CREEP[rate]
    assert moved[0.5] < 5.0 * creep_speed                        # never faster than the capped friction lets it creep
    assert moved[2.0] > 1.0
