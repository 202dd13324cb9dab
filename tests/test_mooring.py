"""Mooring lines (hydro_mooring_wrench, hydro_step_fused_tiled_multi_moor; silver2_isaacsim_amd.mooring.Mooring) as far as a
machine without a GPU can see them: the C boundary, the Python host's marshalling (with the stand-ins of
tests/test_engine_calls.py), ClosedLoopSim's bookkeeping with a fake engine, the host restatement against the fp64 reference
of tests/mooring_reference.py and cases worked by hand, and the physics - config 1's buoy on a line in still water and in a
current - through closed_loop_reference.closed_loop.

THE FIGURES (config 1's buoy: a unit cube of 500 kg in water of 1025 kg/m^3, dt = 1/60, implicit drag, the anchor 20 m below
the buoy's equilibrium position, the fairlead at the centre, k = 0.004 m / dt^2 = 7200 N/m, c = 0.02 m / dt = 600 N s/m):
  still water, L0 = 19 m (1 m short): after 1800 steps |v| = 1.4e-7 m/s, z = -0.405069 m (analytic -0.405069), T = 4195.70 N
      against rho g (0.5 - z) - m g = 4195.70 N
  0.5 m/s current, L0 = 20.5 m: over steps 3000 .. 3600 x = 5.123 m, T = 604.0 N +- 1 N, mean line F_x = -150.34 N against a
      mean hydrodynamic f_x of +150.34 N, never slack; |omega| keeps oscillating (peak to peak 0.15 rad/s) with and without the
      line - the parent's physics - so nothing here asks for omega -> 0 in a current
  the same scene without a line: x = 26.9 m after 3600 steps."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import mooring_reference as mr
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd.mooring import Mooring
from silver2_isaacsim_amd.sea import SeaState
from engine_stand_ins import BODIES, eng, FUSED_HEAD, H, KE, lib, LINES, moor_sim as _sim, N, P13, refused, S, SO, STREAM, T, TILES, _without_lines  # noqa: F401  (fixtures are requested by name)
from mooring_population import ALL_TILE, buoy, CLAMPED, DEPTH, designed_population, NONE_TILE, population_report, TIE_ULPS, TIES
from mooring_reference import PROBE_BOUND

ENTRIES = ("hydro_mooring_wrench", "hydro_step_fused_tiled_multi_moor")
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
W = T((TILES, 6, 64), 0x98000000)                                 # the probe's output
M = T((TILES, 9, 64), 0xA0000000)                                 # the mooring record


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "hydro_mooring_wrench, hydro_step_fused_tiled_multi_moor" in text.split("#define HYDRO_VERSION")[0]   # the version comment
    assert int(re.search(r"#define HYDRO_MOOR_FIELDS\s+(\d+)", code).group(1)) == nat.MOOR_FIELDS == mr.FIELDS == 9
    # the bed entry's argument list with `mooring`, `mooring_tile_stride` in front of step0
    bed, moor = (nat.SIGNATURES["hydro_step_fused_tiled_multi_" + k][1] for k in ("bed", "moor"))
    assert moor == bed[:-2] + [ctypes.c_void_p, ctypes.c_int64] + bed[-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    tail = "int64_t step0, void *stream"
    assert proto("hydro_step_fused_tiled_multi_bed").endswith(tail)
    assert proto("hydro_step_fused_tiled_multi_moor") == (proto("hydro_step_fused_tiled_multi_bed")[:-len(tail)]
                                                          + "const float *mooring, int64_t mooring_tile_stride, " + tail)
    assert proto("hydro_mooring_wrench") == ("hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, const float *mooring, "
                                             "int64_t mooring_tile_stride, float *out, int64_t out_tile_stride, void *stream")
    # the header fixes the record, the rule of thumb, what the kernel does with values it does not validate, and what is not modelled
    for phrase in ("a(3)   anchor, world frame", "b(3)   fairlead, body frame", "tile stride\n * mooring_tile_stride >= 576",
                   "READ AT EVERY LAUNCH", "k dt^2 / m <= 0.04 and c dt / m <= 0.04", "never the one\n * relative to the water",
                   "+0 is NOT added", "computed as given", "the line's mass and catenary sag", "drag on the line", "the line lying on the bed",
                   "more than one line per\n * body", "a line between two bodies"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_moor(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                                None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 576, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_mooring_wrench(None, 64, None, 832, None, 576, None, 384, None) == -1


# ---- the helper ------------------------------------------------------------------------------------------------------------------
def test_mooring_builds_the_record_and_refuses_bad_values():
    m = Mooring([[1, 2, -20], [3, 4, -30]], fairlead=(0.1, 0.0, -0.5), length=[19.0, 29.0], stiffness=7200.0, damping=600.0)
    assert m.n == 2 and m.record.shape == (2, 9) and m.record.dtype == np.float64
    assert m.record.tolist() == [[1, 2, -20, 0.1, 0.0, -0.5, 19.0, 7200.0, 600.0], [3, 4, -30, 0.1, 0.0, -0.5, 29.0, 7200.0, 600.0]]
    assert Mooring((0, 0, -20), length=0.0, stiffness=0.0, n=3).record.shape == (3, 9)          # every edge that is legal; no damping given
    good = dict(anchor=(0.0, 0.0, -20.0), fairlead=(0.0, 0.0, 0.0), length=19.0, stiffness=7200.0, damping=600.0)
    nan, inf = float("nan"), float("inf")
    for key in ("length", "stiffness", "damping"):
        for bad in (nan, inf, -inf):
            with pytest.raises(ValueError, match="non-finite"):
                Mooring(**{**good, key: bad})
        with pytest.raises(ValueError, match=">= 0"):
            Mooring(**{**good, key: -1e-9})
    for key in ("anchor", "fairlead"):
        with pytest.raises(ValueError, match="non-finite"):
            Mooring(**{**good, key: (0.0, nan, 0.0)})
        with pytest.raises(ValueError, match=r"\(3,\) or \(n, 3\)"):
            Mooring(**{**good, key: (0.0, 1.0)})
    with pytest.raises(ValueError, match="does not fit 2 bodies"):
        Mooring([[0, 0, -20], [0, 0, -20]], length=[1.0, 2.0, 3.0], stiffness=1.0)


def test_for_body_gives_the_documented_defaults_and_its_rule_refuses_a_stiff_line():
    for dt in (1 / 60, 1 / 120):
        for mass in (2.0, 500.0):
            k, c = Mooring.for_body(mass, dt)
            assert k * dt * dt / mass == pytest.approx(0.004, rel=1e-14) and c * dt / mass == pytest.approx(0.02, rel=1e-14)
            Mooring((0, 0, -20), length=19.0, stiffness=k, damping=c).check_stable(mass, dt)
            Mooring((0, 0, -20), length=19.0, stiffness=10 * k, damping=2 * c).check_stable(mass, dt)          # the bound itself
    k, c = Mooring.for_body(np.array([2.0, 500.0]), 1 / 60)
    assert k.shape == c.shape == (2,) and k[1] == pytest.approx(7200.0) and c[1] == pytest.approx(600.0)
    dt, mass = 1 / 60, 500.0
    # STABILITY: k dt^2 / m = 1 (and, separately, c dt / m = 1) is rejected by the rule, not silently accepted
    with pytest.raises(ValueError, match=r"k dt\^2 / m = 1"):
        Mooring((0, 0, -20), length=19.0, stiffness=mass / dt ** 2, damping=0.0).check_stable(mass, dt)
    with pytest.raises(ValueError, match="c dt / m = 1"):
        Mooring((0, 0, -20), length=19.0, stiffness=0.0, damping=mass / dt).check_stable(mass, dt)
    with pytest.raises(ValueError, match="body 1"):
        Mooring([[0, 0, -20]] * 2, length=19.0, stiffness=[7200.0, 7200.0 * 11], damping=0.0).check_stable(mass, dt)
    for bad in (dict(mass=0.0, dt=dt), dict(mass=-1.0, dt=dt), dict(mass=500.0, dt=0.0)):
        with pytest.raises(ValueError):
            Mooring.for_body(**bad)


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_mooring_wrench(lib, eng):
    assert eng.mooring_wrench(S, M, N, out=W, stream=STREAM) is W
    assert lib.calls == [("hydro_mooring_wrench", (H, 1000, 0x10000000, 832, 0xA0000000, 576, 0x98000000, 384, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.mooring_wrench, S, M, N, out=C, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 9, 64) tensor on cuda:0", eng.mooring_wrench, S, A, N, out=W, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.mooring_wrench, A, M, N, out=W, stream=STREAM)


def test_step_fused_tiled_multi_moor(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    line = (0xA0000000, 576)
    cases = [(M, dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + line + (0, STREAM)),
             (M, dict(control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + line
              + (123456789012, STREAM)),
             (M, dict(applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + line + (5, STREAM)),
             # no lines: NULL and stride 0, and the library dispatches to the bed entry's launch
             (None, dict(control=C), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, 0x90000000, 1088) + (None, 0) + (9, STREAM))]
    for mooring, kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_moor(S, P13, N, 0.01, 7, step0, mooring, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [("hydro_step_fused_tiled_multi_moor", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_moor, S, P13, N, 0.01, 3, 0, M, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 9, 64) tensor on cuda:0", eng.step_fused_tiled_multi_moor, S, P13, N, 0.01, 3, 0, C, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 17, 64) tensor on cuda:0", eng.step_fused_tiled_multi_moor, S, P13, N, 0.01, 3, 0, M, A, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=5)),
                         ids=lambda c: "".join(n for n, on in zip(("rec", "App", "Ctl", "Sea", "Bed"), c) if on) or "plain")
def test_the_mooring_entry_is_picked_with_every_combination_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, sea, bed = combo
    s = _sim(monkeypatch, *combo)
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert before == [_without_lines(*combo, eager=run != "resident")] * 3
    s.engine.calls.clear()
    s.steps_done = 0
    buf = s.set_mooring(**LINES)
    assert buf is s.mooring and tuple(buf.shape) == (2, 9, 64) and s.engine.calls == []
    # the record: the named bodies' lines, nothing for the others
    rows = scenes.from_tiled(buf.numpy(), BODIES)
    assert rows[66].tolist() == [1.0, 2.0, -20.0, 0.0, np.float32(0.1), -0.5, 19.0, 7200.0, 600.0]
    assert rows[3].tolist() == [3.0, 4.0, -21.0, 0.0, np.float32(0.1), -0.5, 20.0, 7200.0, 600.0]
    assert not np.delete(rows, [66, 3], axis=0).any()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "moor" and call["steps"] == k and call["step0"] == done and call["mooring"] is buf
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the lines were set)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_mooring()
    assert s.mooring is None and s.engine.calls == []
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.clear_mooring()                                              # a second clear is nothing
    assert len(s.engine.calls) == 3
    assert s.set_mooring(**LINES) is buf                           # the buffer's address never changes


def test_graph_replays_take_lines_and_a_current_and_refuse_waves(monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s = _sim(monkeypatch)
    s._graph = "a captured graph without lines"
    s.set_mooring(**LINES)
    assert s._graph is None                                      # captured launches are of another entry
    s._graph = "a captured graph with lines"
    s.set_mooring(**LINES)
    assert s._graph == "a captured graph with lines"            # new contents, the same entry and buffer: the capture stands
    s._graph = None
    s.sea = SeaState((0.3, 0.0, 0.0))
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]
    s.sea = SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [32] and s.steps_done == 0
    s._graph = "a captured graph with lines"
    s.clear_mooring()
    assert s._graph is None


def test_set_mooring_refusals(monkeypatch):
    s = _sim(monkeypatch)
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_mooring(**LINES)
    s.fused = True
    with pytest.raises(ValueError, match="bodies must be in 0 .. 69"):
        s.set_mooring(**{**LINES, "bodies": [3, 70]})
    with pytest.raises(ValueError, match=">= 0"):
        s.set_mooring(**{**LINES, "damping": -1.0})
    with pytest.raises(ValueError, match=r"k dt\^2 / m = 1"):     # the stability rule, for the bodies' own masses
        s.set_mooring(**{**LINES, "stiffness": 500.0 * 3600.0})
    with pytest.raises(ValueError, match="fp32 range"):
        s.set_mooring(**{**LINES, "anchor": (1e39, 0.0, 0.0), "stiffness": 0.0})
    assert s.mooring is None and s.engine.calls == []


# ---- the host restatement ------------------------------------------------------------------------------------------------------------
def _random_lines(n, seed):
    """Bodies with random poses and velocities, a third each: taut, slack, without a line."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 13))
    st[:, 0:3] = rng.uniform(-50, 50, (n, 3))
    q = rng.normal(size=(n, 4))
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))          # non-unit included
    st[:, 7:13] = rng.uniform(-1, 1, (n, 6))
    rec = np.zeros((n, 9))
    rec[:, 0:3] = st[:, 0:3] + rng.uniform(-30, 30, (n, 3))
    rec[:, 3:6] = rng.uniform(-0.6, 0.6, (n, 3))
    l = mr.geometry(rec, st)[2]
    kind = np.arange(n) % 3
    barely = np.arange(n) % 6 == 0                                 # every other taut line is stretched by less than 1e-3 of its length:
    rec[:, 6] = np.where(kind == 0, l * np.where(barely, rng.uniform(0.999, 0.9999, n), rng.uniform(0.9, 0.999, n)),   # the damper decides
                         l * rng.uniform(1.001, 1.2, n))
    rec[:, 7] = np.where(kind == 2, 0.0, rng.uniform(100, 8000, n))
    rec[:, 8] = np.where(kind == 2, 0.0, rng.uniform(0, 600, n))
    return st, rec


def test_host_restatement_equals_the_reference():
    st, rec = _random_lines(600, 23)
    lines = Mooring(rec[:, 0:3], rec[:, 3:6], length=rec[:, 6], stiffness=rec[:, 7], damping=rec[:, 8])
    ref, got, on = mr.wrench(rec, st), lines.wrench(st), mr.taut(rec, st)
    assert on[0::3].all() and not on[1::3].any() and not on[2::3].any()
    pulling = mr.tension(rec, st) > 0
    assert pulling.sum() > 150 and (on & ~pulling).sum() > 3       # some taut lines are clamped: their fairlead closes in too fast
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(ref).max() > 1000.0
    assert not got[~pulling].any() and np.abs(lines.tension(st) - mr.tension(rec, st)).max() <= 1e-12 * mr.tension(rec, st).max()
    # F pulls the fairlead towards the anchor
    _, e, _, _, _, _ = mr.geometry(rec, st)
    assert ((got[pulling, 0:3] * e[pulling]).sum(axis=1) > 0).all()


def test_the_header_s_fp32_order_stands_within_the_probe_bound_of_fp64():
    """The operations include/hydro.h lists, carried out in NumPy float32 (mooring_reference.wrench_fp32_emulated), against the
    fp64 reference with the same lines taut, in units of 2^-24 of mooring_reference.wrench_scales: what the stated order costs
    before any hardware is involved."""
    st, rec = (a.astype(np.float32) for a in _random_lines(600, 23))
    on = mr.taut_fp32(rec, st)
    assert (on == mr.taut(rec, st)).all()                          # no ties in this population (the margins are 1e-3)
    got, ref, scale = mr.wrench_fp32_emulated(rec, st), mr.wrench(rec, st, on), mr.wrench_scales(rec, st, on)
    pulling = mr.tension(rec, st, on) > 0
    assert not got[~pulling].any() and pulling.sum() > 150
    err = np.abs(got[pulling] - ref[pulling]) / (mr.ULP * scale[pulling])
    print(f"[mooring, fp32 order emulated on the host] force {err[:, 0:3].max():.2f}  torque {err[:, 3:6].max():.2f} units of 2^-24 of the scale")
    assert err.max() <= PROBE_BOUND


# ---- the designed population of tests/test_mooring_gpu.py ---------------------------------------------------------------------------


def test_the_designed_population_and_the_probe_bound_on_the_host():
    """The population of the device tests, checked where no device is needed, and the header's fp32 order over it against
    fp64 (ties aside), in units of 2^-24 of the scale: PROBE_BOUND is the next power of two at or above twice the largest."""
    st, _, pr, rec = designed_population()
    pulling, slack, none, clamped = population_report(rec, st)
    off = ~np.isin(np.arange(321), TIES)
    assert (mr.taut_fp32(rec, st) == mr.taut(rec, st))[off].all()                 # the emulation agrees with the reference off the ties
    for n in (200, 321):
        assert pulling[:n].mean() >= 0.25 and slack[:n].mean() >= 0.25 and none[:n].mean() >= 0.25, (n, pulling[:n].sum(), slack[:n].sum(), none[:n].sum())
    assert none[64 * NONE_TILE:64 * NONE_TILE + 64].all() and mr.taut(rec, st)[64 * ALL_TILE:64 * ALL_TILE + 64].all()
    assert pulling[320] and clamped[CLAMPED].all() and clamped.sum() >= 8
    # over the bed of tests/test_seabed_gpu.py every combination of "touches" and "pulls" occurs, at either size
    import seabed_reference as br
    from designed_populations import BED as STEP_BED
    touches = br.touching_fp32(STEP_BED, st, pr).any(axis=1)
    for n in (200, 321):
        classes = [(touches & pulling)[:n].sum(), (touches & ~pulling)[:n].sum(), (pulling & ~touches)[:n].sum(), (~pulling & ~touches)[:n].sum()]
        assert min(classes) >= 8, (n, classes)
    free = rec.copy()
    free[:, 6] = 0
    l32 = mr._fp32_terms(free, st)[3]
    ulps = (rec[TIES, 6].astype(np.float64) - l32[TIES]) / np.spacing(l32[TIES])
    assert ulps.tolist() == list(TIE_ULPS) and not rec[TIES[:4], 8].any() and (rec[TIES[4:], 8] > 0).all()
    assert (mr.geometry(rec, st)[5][TIES] < 0).all()                              # running away: a taut tie with a damper pulls
    on = mr.taut_fp32(rec, st)
    got, ref, scale = mr.wrench_fp32_emulated(rec, st), mr.wrench(rec, st, on), mr.wrench_scales(rec, st, on)
    live = (mr.tension(rec, st, on) > 0) & off
    assert not got[~live & off].any()
    err = np.abs(got[live] - ref[live]) / (mr.ULP * scale[live])
    print(f"[mooring, designed population, fp32 order emulated on the host] force {err[:, 0:3].max():.2f}  torque {err[:, 3:6].max():.2f} "
          f"units of 2^-24 of the scale (bound {PROBE_BOUND:g})")
    assert err.max() <= PROBE_BOUND


def _one(anchor, fairlead, L0, k, c, p=(0, 0, 0), q=(0, 0, 0, 1), v=(0, 0, 0), om=(0, 0, 0)):
    st = np.zeros((1, 13))
    st[0, 0:3], st[0, 3:7], st[0, 7:10], st[0, 10:13] = p, q, v, om
    rec = np.array([[*anchor, *fairlead, L0, k, c]], np.float64)
    lines = Mooring(rec[:, 0:3], rec[:, 3:6], length=rec[:, 6], stiffness=rec[:, 7], damping=rec[:, 8])
    return lines.wrench(st)[0], mr.wrench(rec, st)[0], bool(mr.taut(rec, st)[0])


def test_lines_by_hand():
    # a vertical taut line through the centre: 20 m to the anchor, 19 m of line, k = 100 -> 100 N straight down, no torque
    for got in _one((0, 0, -20), (0, 0, 0), 19.0, 100.0, 0.0)[:2]:
        assert got == pytest.approx([0, 0, -100.0, 0, 0, 0], abs=1e-12)
    # ... and sinking at 0.5 m/s towards the anchor with c = 40: T = 100 - 40 * 0.5 = 80
    for got in _one((0, 0, -20), (0, 0, 0), 19.0, 100.0, 40.0, v=(0, 0, -0.5))[:2]:
        assert got == pytest.approx([0, 0, -80.0, 0, 0, 0], abs=1e-12)
    # an offset fairlead: b = (0.5, 0, 0), the anchor straight below it, 10 m down, 9 m of line, k = 50 -> F = (0, 0, -50) at
    # r = (0.5, 0, 0): r x F = (0, 0.5 * 50, 0) = (0, 25, 0)
    for got in _one((0.5, 0, -10), (0.5, 0, 0), 9.0, 50.0, 0.0)[:2]:
        assert got == pytest.approx([0, 0, -50.0, 0, 25.0, 0], abs=1e-12)
    # the same body turned a quarter about z (q = (0, 0, sin 45, cos 45)): the fairlead stands at (0, 0.5, 0); the anchor at
    # (3, 0.5, -4) is 5 m away, 4 m of line, k = 10 -> T = 10, F = (6, 0, -8), r x F = (0.5 * -8, 0, -0.5 * 6) = (-4, 0, -3)
    h = np.sqrt(0.5)
    for got in _one((3, 0.5, -4), (0.5, 0, 0), 4.0, 10.0, 0.0, q=(0, 0, h, h))[:2]:
        assert got == pytest.approx([6.0, 0, -8.0, -4.0, 0, -3.0], abs=1e-12)
    # spinning about z at 2 rad/s the fairlead at (0, 0.5, 0) moves at omega x r = (-1, 0, 0): un = (-1, 0, 0) . (3, 0, -4) / 5 =
    # -0.6 (it runs away from the anchor), c = 5 adds 3 N: T = 13
    for got in _one((3, 0.5, -4), (0.5, 0, 0), 4.0, 10.0, 5.0, q=(0, 0, h, h), om=(0, 0, 2.0))[:2]:
        assert got == pytest.approx(np.array([6.0, 0, -8.0, -4.0, 0, -3.0]) * 1.3, abs=1e-12)
    # a slack line gives nothing, whatever the fairlead does
    got, ref, on = _one((0, 0, -20), (0, 0, 0), 20.5, 100.0, 40.0, v=(0, 0, 3.0))
    assert not on and not got.any() and not ref.any()
    # an approaching fairlead with c large: taut by 1 m (100 N of spring) but closing in at 0.5 m/s with c = 400 -> T clamped to 0
    got, ref, on = _one((0, 0, -20), (0, 0, 0), 19.0, 100.0, 400.0, v=(0, 0, -0.5))
    assert on and not got.any() and not ref.any()
    # the fairlead on the anchor (l = 0): not taut, nothing, and no NaN
    got, ref, on = _one((0, 0, -20), (0, 0, 0), 0.0, 100.0, 40.0, p=(0, 0, -20))
    assert not on and not got.any() and not ref.any()
    # no line (k = c = 0): nothing, though the geometry is stretched
    got, ref, on = _one((0, 0, -20), (0, 0, 0), 19.0, 0.0, 0.0)
    assert not on and not got.any() and not ref.any()


# ---- the physics: config 1's buoy on a line --------------------------------------------------------------------------------------------


def test_still_water_a_short_line_pulls_the_buoy_down_to_the_analytic_depth():
    st, pv, pr, sc, dt, z_eq, mass = buoy()
    k, c = Mooring.for_body(mass, dt)
    lines = Mooring((0.0, 0.0, z_eq - DEPTH), length=DEPTH - 1.0, stiffness=k, damping=c)          # 1 m short
    lines.check_stable(mass, dt)
    run = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 1800, moor=lines.record, implicit=True)
    s = run[-1]["state"][0].astype(np.float64)
    # rho g A (0.5 - z) - m g = k ((z - z_anchor) - L0), A = 1 m^2: linear in z
    z_want = (sc.rho * sc.g * 0.5 - mass * sc.g - k * (DEPTH - z_eq - (DEPTH - 1.0))) / (sc.rho * sc.g + k)
    speed, T = float(np.linalg.norm(s[7:10])), float(run[-1]["tension"][0])
    print(f"[still water] |v| {speed:.2e} m/s  z {s[2]:+.6f} m (analytic {z_want:+.6f})  T {T:.2f} N  rho g (0.5 - z) - m g {sc.rho * sc.g * (0.5 - s[2]) - mass * sc.g:.2f} N")
    assert speed < 1e-5
    assert abs(s[2] - z_want) < 1e-4 and z_want < z_eq - 0.05      # and it was pulled down
    assert abs(T - (sc.rho * sc.g * (0.5 - s[2]) - mass * sc.g)) < 0.1
    assert all(r["taut"][0] for r in run)


@pytest.fixture(scope="module")
def in_a_current():
    """The buoy in a 0.5 m/s current for 3600 steps, moored (centre fairlead, default constants, 20.5 m of line) and adrift."""
    st, pv, pr, sc, dt, z_eq, mass = buoy()
    k, c = Mooring.for_body(mass, dt)
    lines = Mooring((0.0, 0.0, z_eq - DEPTH), length=DEPTH + 0.5, stiffness=k, damping=c)
    sea = SeaState((0.5, 0.0, 0.0))
    moored = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 3600, moor=lines.record, sea=sea, implicit=True)
    adrift = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 3600, sea=sea, implicit=True)
    return lines, moored, adrift


def test_current_the_line_holds_the_buoy_on_station(in_a_current):
    lines, moored, _ = in_a_current
    reach = np.array([mr.geometry(lines.record, r["state"])[2][0] for r in moored])
    last = moored[-600:]
    line_fx = np.mean([r["line"][0, 0] for r in last])
    hydro_fx = np.mean([r["hydro"][0, 0] for r in last])
    T = np.array([r["tension"][0] for r in last])
    x = np.array([r["state"][0, 0] for r in last], np.float64)
    print(f"[current] x {x.mean():.3f} m (ptp {np.ptp(x):.1e})  T {T.mean():.1f} N (ptp {np.ptp(T):.2f})  line F_x {line_fx:.2f} N  "
          f"hydrodynamic f_x {hydro_fx:.2f} N  longest {reach.max():.3f} m of {lines.record[0, 6]} m")
    # within the line's reach: never stretched by more than 1 % (the stretch that carries the load is T / k = 0.08 m)
    assert reach.max() < 1.01 * lines.record[0, 6]
    assert hydro_fx > 50.0 and abs(-line_fx - hydro_fx) <= 0.05 * hydro_fx
    assert all(r["taut"][0] and r["tension"][0] > 0 for r in last)  # never slack there
    assert 1.0 < x.mean() < 10.0                                   # downstream of the anchor, on station


def test_drift_without_a_line_the_buoy_leaves(in_a_current):
    _, moored, adrift = in_a_current
    gone = float(adrift[-1]["state"][0, 0])
    print(f"[drift] x {gone:.1f} m after 3600 steps without a line, {float(moored[-1]['state'][0, 0]):.2f} m with it")
    assert gone > 20.0
