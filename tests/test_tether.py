"""Tethers (hydro_tether_wrench, hydro_step_fused_tiled_multi_teth; silver2_isaacsim_amd.tether.Tether) as far as a machine
without a GPU can see them: the C boundary, the Python host's marshalling (with the stand-ins of tests/test_engine_calls.py),
ClosedLoopSim's bookkeeping with a fake engine under its three runners and all 128 combinations of recorder, applied wrench,
pose hold, sea, bed, mooring lines and extremes, every refusal of Tether and set_tether, the host restatement against the fp64
reference of tests/tether_reference.py and cases worked by hand, the exact antisymmetry of the header's fp32 order, the
designed population of tests/test_tether_gpu.py with the probe bound that stands on it, and two physical cases through
closed_loop_reference.closed_loop.

THE PROBE BOUND (tests/test_tether_gpu.py asserts it on the device).  Errors of the header's order emulated on the host in
fp32 (tether_reference.wrench_fp32_emulated: a correctly rounded seed for the reciprocal square root) against
tether_reference.wrench (fp64), in units of 2^-24 of tether_reference.wrench_scales, over the designed population at n = 200,
321 and 322, the sixteen bodies at the tie aside: force 0.90, torque 0.48, tension 0.90 (test_the_designed_population_and_the_probe_bound_on_the_host
prints them).  The rule of DESIGN.md sections 17 - 20: the next power of two at or above twice the largest, 2 x 0.90 = 1.80 ->
PROBE_BOUND = 2.

THE FIGURES of the physical cases (dt = 1/60, implicit drag, water of 1025 kg/m^3):
  a box of 0.5 m and 200 kg on 5 m of line under config 1's buoy (a unit cube of 500 kg), centre fairleads, the default
      constants of the pair: after 2400 steps |v| <= 3e-6 m/s on both, T = 705.10 N against the box's submerged weight
      (m - rho V) g = (200 - 128.125) 9.81 = 705.09 N
  a free pair (no water, no gravity) of 3 kg and 7 kg with offset fairleads, parting at 1.2 m/s on a line 0.2 m short: over 240
      steps the total momentum moves by no more than the rounding of the velocity additions, the bound the test forms"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import tether_reference as tr
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd import tether as th
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.tether import Tether
from engine_stand_ins import (BODIES, eng, ext_sim as _ext_sim, ExtEngine, FUSED_HEAD, H, KE, lib, LINES, N, P13, refused, S, SO, STREAM, T, TILES,
                              _without_extremes)  # noqa: F401  (fixtures are requested by name)
from tether_population import assert_antisymmetric, bodies_of, check_population, designed_population, hanging_pair, LINE, record_for, SIZES
from tether_reference import PROBE_BOUND

ENTRIES = ("hydro_tether_wrench", "hydro_step_fused_tiled_multi_teth")
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
W = T((TILES, 6, 64), 0x98000000)                                 # the probe's output
M = T((TILES, 9, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)
TT = T((TILES, 7, 64), 0xB0000000)                                # the tether record
T1 = T((TILES, 1, 64), 0xB8000000)                                # the probe's tension


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "hydro_tether_wrench, hydro_step_fused_tiled_multi_teth" in text.split("#define HYDRO_VERSION")[0]     # the version comment
    assert int(re.search(r"#define HYDRO_TETH_FIELDS\s+(\d+)", code).group(1)) == nat.TETH_FIELDS == tr.FIELDS == th.FIELDS == 7
    # the extremes entry's argument list with `tether`, `tether_tile_stride` in front of step0
    ext, teth = (nat.SIGNATURES["hydro_step_fused_tiled_multi_" + k][1] for k in ("ext", "teth"))
    assert teth == ext[:-2] + [ctypes.c_void_p, ctypes.c_int64] + ext[-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    tail = "int64_t step0, void *stream"
    assert proto("hydro_step_fused_tiled_multi_teth") == (proto("hydro_step_fused_tiled_multi_ext")[:-len(tail)]
                                                          + "const float *tether, int64_t tether_tile_stride, " + tail)
    assert proto("hydro_tether_wrench") == ("hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, const float *tether, "
                                            "int64_t tether_tile_stride, float *out, int64_t out_tile_stride, float *tension, "
                                            "int64_t tension_tile_stride, void *stream")
    # the header fixes the record, the scope, what a malformed record does, the order, the tested property and what is not modelled
    for phrase in ("b(3)     this body's fairlead", "partner  the other body, as a LANE INDEX WITHIN THE SAME TILE", "tether_tile_stride >= 448",
                   "READ IN EVERY STEP", "at most one tether per body", "both bodies of a pair in one tile", "an\n * involution",
                   "carry the same L0, k, c", "NO PARTNER INDEX EVER FORMS A MEMORY ADDRESS", "(int)partner & 63", "computed as given and cannot fault",
                   "names an unspecified lane of the tile and still never an address",
                   "never the one\n * relative to the water", "P_i    = p_i + r_i", "e_i    = P'_i - P_i", "T      = max(0, fma(k, x, c * rate))",
                   "+0 is NOT added", "EQUAL AND OPPOSITE, EXACTLY (a property that is tested)", "negation is exact in fp32",
                   "chains, and more than one tether per body", "pairs across tiles", "the line's mass, sag and drag",
                   "tension_max stays the mooring line's", "k dt^2 / mu <= 0.04 and c dt / mu <= 0.04"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_teth(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                                None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 576,
                                                None, 512, None, 448, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_tether_wrench(None, 64, None, 832, None, 448, None, 384, None, 64, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_tether_wrench(lib, eng):
    assert eng.tether_wrench(S, TT, N, out=W, stream=STREAM) is W
    assert eng.tether_wrench(S, TT, N, out=W, tension=T1, stream=STREAM) is W
    assert lib.calls == [("hydro_tether_wrench", (H, 1000, 0x10000000, 832, 0xB0000000, 448, 0x98000000, 384, None, 0, STREAM)),
                         ("hydro_tether_wrench", (H, 1000, 0x10000000, 832, 0xB0000000, 448, 0x98000000, 384, 0xB8000000, 64, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.tether_wrench, S, TT, N, out=C, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 7, 64) tensor on cuda:0", eng.tether_wrench, S, A, N, out=W, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.tether_wrench, A, TT, N, out=W, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 1, 64) tensor on cuda:0", eng.tether_wrench, S, TT, N, out=W, tension=A, stream=STREAM)


def test_step_fused_tiled_multi_teth(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    line, record, tether = (0xA0000000, 576), (0xA8000000, 512), (0xB0000000, 448)
    cases = [(TT, dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0) + (None, 0) + tether + (0, STREAM)),
             (TT, dict(extremes=E, mooring=M, control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + line + record + tether
              + (123456789012, STREAM)),
             # `tether` in front of step0, behind the extremes
             (TT, dict(extremes=E, applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0) + record + tether + (5, STREAM)),
             # no tethers: NULL and stride 0, and the library dispatches to the extremes entry's launch
             (None, dict(mooring=M, control=C), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, 0x90000000, 1088) + line + (None, 0) + (None, 0) + (9, STREAM))]
    for tether_, kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_teth(S, P13, N, 0.01, 7, step0, tether_, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [("hydro_step_fused_tiled_multi_teth", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_teth, S, P13, N, 0.01, 3, 0, TT, E, M, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 7, 64) tensor on cuda:0", eng.step_fused_tiled_multi_teth, S, P13, N, 0.01, 3, 0, M, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 8, 64) tensor on cuda:0", eng.step_fused_tiled_multi_teth, S, P13, N, 0.01, 3, 0, TT, M, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 9, 64) tensor on cuda:0", eng.step_fused_tiled_multi_teth, S, P13, N, 0.01, 3, 0, TT, E, E, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class TethEngine(ExtEngine):
    """tests/test_extremes.py's recording engine with the new call."""

    def step_fused_tiled_multi_teth(self, cur, old, n, dt, steps, step0, tether, extremes, mooring, control, applied, frame, implicit_drag=False,
                                    ke_out=None, log=None, **rec):
        return self._step("teth", cur, steps, step0=step0, tether=tether, extremes=extremes, mooring=mooring, control=control, applied=applied,
                          frame=frame, log=log)


def _sim(monkeypatch, recorder=False, applied=False, control=False, sea=False, bed=False, lines=False, extremes=False):
    s = _ext_sim(monkeypatch, recorder, applied, control, sea, bed)
    s.engine = TethEngine()
    if lines:
        s.set_mooring(**LINES)
    if extremes:
        s.track_extremes()
        s.engine.calls.clear()
    return s


PAIRS = dict(pairs=[[66, 69], [3, 40]], fairlead_a=[[0.0, 0.1, -0.5], [0.2, 0.0, 0.0]], fairlead_b=(0.0, 0.0, 0.25), length=[5.0, 6.0],
             stiffness=1800.0, damping=150.0)


def _without_tether(recorder, applied, control, sea, bed, lines, extremes, eager):
    return "ext" if extremes else _without_extremes(recorder, applied, control, sea, bed, lines, eager)


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=7)),
                         ids=lambda c: "".join(n for n, on in zip(("rec", "App", "Ctl", "Sea", "Bed", "Moor", "Ext"), c) if on) or "plain")
def test_the_tether_entry_is_picked_with_every_combination_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, sea, bed, lines, extremes = combo
    s = _sim(monkeypatch, *combo)
    assert simulate.ClosedLoopSim.tether is None and s.tether is None            # a class default: a sim has no tethers until some are set
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert before == [_without_tether(*combo, eager=run != "resident")] * 3
    s.engine.calls.clear()
    s.steps_done = 0
    buf = s.set_tether(**PAIRS)
    assert buf is s.tether and tuple(buf.shape) == (2, 7, 64) and s.engine.calls == []
    # the record: both bodies of a pair carry the line's constants and each other's lane, everybody else names itself
    rows = scenes.from_tiled(buf.numpy(), BODIES)
    assert rows[66].tolist() == [0.0, np.float32(0.1), -0.5, 5.0, 1800.0, 150.0, 5.0] and rows[69].tolist() == [0.0, 0.0, 0.25, 5.0, 1800.0, 150.0, 2.0]
    assert rows[3].tolist() == [np.float32(0.2), 0.0, 0.0, 6.0, 1800.0, 150.0, 40.0] and rows[40].tolist() == [0.0, 0.0, 0.25, 6.0, 1800.0, 150.0, 3.0]
    others = np.delete(np.arange(BODIES), [66, 69, 3, 40])
    assert not rows[others, 0:6].any() and rows[others, 6].tolist() == (others % 64).tolist()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "teth" and call["steps"] == k and call["step0"] == done and call["tether"] is buf
        assert call["extremes"] is (s.extremes.buffer if extremes else None)
        assert call["mooring"] is s.mooring and (s.mooring is not None) == lines
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the tethers were set)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_tether()
    assert s.tether is None and s.engine.calls == []
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.clear_tether()                                               # a second clear is nothing
    assert len(s.engine.calls) == 3
    assert s.set_tether(**PAIRS) is buf                            # the buffer's address never changes


def test_graph_replays_take_tethers_and_a_current_and_refuse_waves(monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s = _sim(monkeypatch, lines=True)
    s._graph = "a captured graph without tethers"
    s.set_tether(**PAIRS)
    assert s._graph is None                                      # captured launches are of another entry
    s._graph = "a captured graph with tethers"
    s.set_tether(**PAIRS)
    assert s._graph == "a captured graph with tethers"          # new contents, the same entry and buffer: the capture stands
    s._graph = None
    s.sea = SeaState((0.3, 0.0, 0.0))
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]
    s.sea = SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [32] and s.steps_done == 0
    s._graph = "a captured graph with tethers"
    s.clear_tether()
    assert s._graph is None


def test_set_tether_refusals(monkeypatch):
    s = _sim(monkeypatch)
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_tether(**PAIRS)
    s.fused = True
    with pytest.raises(ValueError, match="outside 0 .. 69"):
        s.set_tether(**{**PAIRS, "pairs": [[66, 70], [3, 40]]})
    with pytest.raises(ValueError, match="tiles 0 and 1.*inside one block of 64"):
        s.set_tether(**{**PAIRS, "pairs": [[66, 69], [3, 64]]})
    with pytest.raises(ValueError, match=">= 0"):
        s.set_tether(**{**PAIRS, "damping": -1.0})
    with pytest.raises(ValueError, match=r"k dt\^2 / mu = 1"):    # the stability rule, for the pair's reduced mass (250 kg)
        s.set_tether(**{**PAIRS, "stiffness": 250.0 * 3600.0})
    with pytest.raises(ValueError, match="fp32 range"):
        s.set_tether(**{**PAIRS, "fairlead_b": (1e39, 0.0, 0.0), "stiffness": 0.0})
    assert s.tether is None and s.engine.calls == []


# ---- the helper ------------------------------------------------------------------------------------------------------------------
def test_tether_builds_the_record_and_refuses_bad_values():
    t = Tether([[1, 2], [70, 65]], fairlead_a=(0.1, 0.0, -0.5), fairlead_b=[[0, 0, 1], [0, 0, 2]], length=[19.0, 29.0], stiffness=7200.0, damping=600.0, n=130)
    assert t.n == 130 and t.record.shape == (130, 7) and t.record.dtype == np.float64
    assert t.record[1].tolist() == [0.1, 0.0, -0.5, 19.0, 7200.0, 600.0, 2.0] and t.record[2].tolist() == [0, 0, 1, 19.0, 7200.0, 600.0, 1.0]
    assert t.record[70].tolist() == [0.1, 0.0, -0.5, 29.0, 7200.0, 600.0, 1.0] and t.record[65].tolist() == [0, 0, 2, 29.0, 7200.0, 600.0, 6.0]
    assert t.partner[[1, 2, 70, 65, 0, 129]].tolist() == [2, 1, 65, 70, 0, 129]
    assert (t.partner[t.partner] == np.arange(130)).all()          # an involution
    assert Tether(np.zeros((0, 2), int), length=1.0, stiffness=1.0, n=3).record[:, 0:6].any() == False  # noqa: E712  (nobody tethered is legal)
    assert Tether([0, 1], length=0.0, stiffness=0.0, n=2).record.shape == (2, 7)                 # every edge that is legal; one pair as (2,)
    good = dict(pairs=[[0, 1]], fairlead_a=(0.0, 0.0, 0.0), fairlead_b=(0.0, 0.0, 0.0), length=5.0, stiffness=7200.0, damping=600.0, n=200)
    nan, inf = float("nan"), float("inf")
    for key in ("length", "stiffness", "damping"):
        for bad in (nan, inf, -inf):
            with pytest.raises(ValueError, match="non-finite"):
                Tether(**{**good, key: bad})
        with pytest.raises(ValueError, match=">= 0"):
            Tether(**{**good, key: -1e-9})
    for key in ("fairlead_a", "fairlead_b"):
        with pytest.raises(ValueError, match="non-finite"):
            Tether(**{**good, key: (0.0, nan, 0.0)})
        with pytest.raises(ValueError, match=r"\(3,\) or \(m, 3\)"):
            Tether(**{**good, key: (0.0, 1.0)})
    with pytest.raises(ValueError, match="does not fit 2 pairs"):
        Tether([[0, 1], [2, 3]], length=[1.0, 2.0, 3.0], stiffness=1.0, n=10)
    with pytest.raises(ValueError, match="body 5 is tied to itself"):
        Tether(**{**good, "pairs": [[0, 1], [5, 5]]})
    with pytest.raises(ValueError, match="body 1 is in two pairs"):
        Tether(**{**good, "pairs": [[0, 1], [1, 2]]})
    with pytest.raises(ValueError, match="outside 0 .. 199"):
        Tether(**{**good, "pairs": [[0, 200]]})
    with pytest.raises(ValueError, match="outside 0 .. 199"):
        Tether(**{**good, "pairs": [[-1, 3]]})
    with pytest.raises(ValueError, match=r"bodies 63 and 64 lie in tiles 0 and 1; a pair must lie inside one block of 64 bodies.*lay the pair out inside one block of 64"):
        Tether(**{**good, "pairs": [[63, 64]]})
    with pytest.raises(ValueError, match="tiles 2 and 0"):
        Tether(**{**good, "pairs": [[130, 5]]})
    with pytest.raises(ValueError, match=r"\(m, 2\) integer"):
        Tether(**{**good, "pairs": [[0.0, 1.0]]})
    with pytest.raises(ValueError, match=r"\(m, 2\) integer"):
        Tether(**{**good, "pairs": [[0, 1, 2]]})


def test_for_pair_gives_the_documented_defaults_and_its_rule_refuses_a_stiff_line():
    for dt in (1 / 60, 1 / 120):
        for m_a, m_b in ((2.0, 500.0), (500.0, 500.0)):
            mu = m_a * m_b / (m_a + m_b)
            k, c = Tether.for_pair(m_a, m_b, dt)
            assert k * dt * dt / mu == pytest.approx(0.004, rel=1e-14) and c * dt / mu == pytest.approx(0.02, rel=1e-14)
            Tether([[0, 1]], length=5.0, stiffness=k, damping=c, n=2).check_stable([m_a, m_b], dt)
            Tether([[0, 1]], length=5.0, stiffness=10 * k, damping=2 * c, n=2).check_stable([m_a, m_b], dt)   # the bound itself
    k, c = Tether.for_pair(np.array([2.0, 500.0]), np.array([2.0, 500.0]), 1 / 60)
    assert k.shape == c.shape == (2,) and k[1] == pytest.approx(3600.0) and c[1] == pytest.approx(300.0)
    dt, mass = 1 / 60, 500.0                                      # mu = 250
    with pytest.raises(ValueError, match=r"k dt\^2 / mu = 1"):
        Tether([[0, 1]], length=5.0, stiffness=250.0 / dt ** 2, n=2).check_stable(mass, dt)
    with pytest.raises(ValueError, match="c dt / mu = 1"):
        Tether([[0, 1]], length=5.0, stiffness=0.0, damping=250.0 / dt, n=2).check_stable(mass, dt)
    # the REDUCED mass decides: a line that a 500 kg body alone would carry is too stiff between it and a 2 kg body
    k500, _ = Tether.for_pair(1e9, 500.0, dt)
    with pytest.raises(ValueError, match=r"pair \(2, 3\)"):
        Tether([[0, 1], [2, 3]], length=5.0, stiffness=10 * k500 * 0.99, n=4).check_stable([500.0, 500.0, 500.0, 2.0], dt)
    for bad in (dict(m_a=0.0, m_b=1.0, dt=dt), dict(m_a=1.0, m_b=-1.0, dt=dt), dict(m_a=500.0, m_b=1.0, dt=0.0)):
        with pytest.raises(ValueError):
            Tether.for_pair(**bad)


# ---- the host restatement ------------------------------------------------------------------------------------------------------------
def _random_pairs(n, seed):
    """n bodies (a multiple of 6) with random poses and velocities, in consecutive pairs (2 i, 2 i + 1) - never across a tile, 64
    being even: a third of the pairs each taut, slack, without a tether."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 13))
    st[:, 0:3] = rng.uniform(-50, 50, (n, 3))
    st[1::2, 0:3] = st[0::2, 0:3] + rng.uniform(-30, 30, (n // 2, 3))
    q = rng.normal(size=(n, 4))
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))          # non-unit included
    st[:, 7:13] = rng.uniform(-1, 1, (n, 6))
    rec = np.zeros((n, 7))
    rec[:, 0:3] = rng.uniform(-0.6, 0.6, (n, 3))
    i = np.arange(n)
    rec[:, 6] = (i ^ 1) % 64
    l = tr.geometry(rec, st)[2]
    assert np.array_equal(l[0::2], l[1::2])
    kind = (i // 2) % 3
    barely = (i // 2) % 6 == 0
    per_pair = lambda a: np.repeat(a, 2)  # noqa: E731
    rec[:, 3] = np.where(kind == 0, l * per_pair(np.where(barely[0::2], rng.uniform(0.999, 0.9999, n // 2), rng.uniform(0.9, 0.999, n // 2))),
                         l * per_pair(rng.uniform(1.001, 1.2, n // 2)))
    rec[:, 4] = np.where(kind == 2, 0.0, per_pair(rng.uniform(100, 8000, n // 2)))
    rec[:, 5] = np.where(kind == 2, 0.0, per_pair(rng.uniform(0, 600, n // 2)))
    return st, rec


def _as_tether(rec):
    n = len(rec)
    a = np.arange(0, n, 2)
    return Tether(np.stack([a, a + 1], axis=1), rec[a, 0:3], rec[a + 1, 0:3], length=rec[a, 3], stiffness=rec[a, 4], damping=rec[a, 5], n=n)


def test_host_restatement_equals_the_reference():
    st, rec = _random_pairs(600, 29)
    lines = _as_tether(rec)
    assert np.array_equal(lines.record, rec)
    ref, got, on = tr.wrench(rec, st), lines.wrench(st), tr.taut(rec, st)
    kind = (np.arange(600) // 2) % 3
    assert on[kind == 0].all() and not on[kind != 0].any()
    pulling = tr.tension(rec, st) > 0
    assert pulling.sum() > 150 and (on & ~pulling).sum() > 3       # some taut lines are clamped: the fairleads close in too fast
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(ref).max() > 1000.0
    assert not got[~pulling].any() and np.abs(lines.tension(st) - tr.tension(rec, st)).max() <= 1e-12 * tr.tension(rec, st).max()
    # F pulls the fairlead towards the partner's, and the partner's the other way with the same strength
    _, e, _, _, _, _ = tr.geometry(rec, st)
    assert ((got[pulling, 0:3] * e[pulling]).sum(axis=1) > 0).all()
    assert np.abs(got[0::2, 0:3] + got[1::2, 0:3]).max() <= 1e-12 * np.abs(ref).max()


def _two(fair_a, fair_b, L0, k, c, pa=(0, 0, 0), pb=(0, 0, 0), qa=(0, 0, 0, 1), va=(0, 0, 0), vb=(0, 0, 0), oma=(0, 0, 0)):
    st = np.zeros((2, 13))
    st[0, 0:3], st[1, 0:3], st[0, 3:7], st[1, 3:7], st[0, 7:10], st[1, 7:10], st[0, 10:13] = pa, pb, qa, (0, 0, 0, 1), va, vb, oma
    lines = Tether([[0, 1]], fair_a, fair_b, length=L0, stiffness=k, damping=c, n=2)
    return lines.wrench(st), tr.wrench(lines.record, st), bool(tr.taut(lines.record, st)[0]), lines.tension(st)


def test_tethers_by_hand():
    # two bodies 1 m apart on a 0.5 m line, k = 100: T = 50; a is pulled towards b (+x), b towards a (-x), no torque
    for got in _two((0, 0, 0), (0, 0, 0), 0.5, 100.0, 0.0, pb=(1, 0, 0))[:2]:
        assert got[0] == pytest.approx([50.0, 0, 0, 0, 0, 0], abs=1e-12) and got[1] == pytest.approx([-50.0, 0, 0, 0, 0, 0], abs=1e-12)
    # ... parting at 0.5 m/s with c = 40: T = 50 + 40 * 0.5 = 70, on both
    got, ref, on, T = _two((0, 0, 0), (0, 0, 0), 0.5, 100.0, 40.0, pb=(1, 0, 0), va=(-0.2, 0, 0), vb=(0.3, 0, 0))
    assert got[0] == pytest.approx([70.0, 0, 0, 0, 0, 0], abs=1e-12) and np.allclose(got, ref, atol=1e-12) and T.tolist() == pytest.approx([70.0, 70.0])
    # an offset fairlead: a's fairlead at b_a = (0.5, 0, 0), b straight below it at (0.5, 0, -10), 9 m of line, k = 50:
    # F_a = (0, 0, -50) at r = (0.5, 0, 0): r x F = (0, 0.5 * 50, 0) = (0, 25, 0); b is pulled up through its centre: no torque
    for got in _two((0.5, 0, 0), (0, 0, 0), 9.0, 50.0, 0.0, pb=(0.5, 0, -10))[:2]:
        assert got[0] == pytest.approx([0, 0, -50.0, 0, 25.0, 0], abs=1e-12) and got[1] == pytest.approx([0, 0, 50.0, 0, 0, 0], abs=1e-12)
    # a turned a quarter about z: its fairlead stands at (0, 0.5, 0); b at (3, 0.5, -4) is 5 m away, 4 m of line, k = 10 ->
    # T = 10, F_a = (6, 0, -8), r x F = (0.5 * -8, 0, -0.5 * 6) = (-4, 0, -3); spinning about z at 2 rad/s the fairlead moves at
    # (-1, 0, 0): dU = (1, 0, 0), rate = 3 / 5 = 0.6 (they part), c = 5 adds 3 N: T = 13
    h = np.sqrt(0.5)
    for got in _two((0.5, 0, 0), (0, 0, 0), 4.0, 10.0, 0.0, pb=(3, 0.5, -4), qa=(0, 0, h, h))[:2]:
        assert got[0] == pytest.approx([6.0, 0, -8.0, -4.0, 0, -3.0], abs=1e-12) and got[1] == pytest.approx([-6.0, 0, 8.0, 0, 0, 0], abs=1e-12)
    for got in _two((0.5, 0, 0), (0, 0, 0), 4.0, 10.0, 5.0, pb=(3, 0.5, -4), qa=(0, 0, h, h), oma=(0, 0, 2.0))[:2]:
        assert got[0] == pytest.approx(np.array([6.0, 0, -8.0, -4.0, 0, -3.0]) * 1.3, abs=1e-12)
    # a closing pair: taut by 0.5 m (50 N of spring) but closing at 0.5 m/s with c = 400 -> T clamps to 0
    got, ref, on, T = _two((0, 0, 0), (0, 0, 0), 0.5, 100.0, 400.0, pb=(1, 0, 0), va=(0.5, 0, 0))
    assert on and not got.any() and not ref.any() and not T.any()
    # a slack line gives nothing, whatever the bodies do
    got, ref, on, T = _two((0, 0, 0), (0, 0, 0), 1.5, 100.0, 40.0, pb=(1, 0, 0), vb=(3.0, 0, 0))
    assert not on and not got.any() and not ref.any() and not T.any()
    # the fairleads on each other (l = 0): not taut, nothing, and no NaN
    got, ref, on, T = _two((0.5, 0, 0), (-0.5, 0, 0), 0.0, 100.0, 40.0, pb=(1, 0, 0), vb=(1.0, 0, 0))
    assert not on and not got.any() and not ref.any() and np.isfinite(got).all() and not T.any()
    # no tether (k = c = 0): nothing, though the geometry is stretched
    got, ref, on, T = _two((0, 0, 0), (0, 0, 0), 0.5, 0.0, 0.0, pb=(1, 0, 0))
    assert not on and not got.any() and not ref.any()


# ---- the designed population of tests/test_tether_gpu.py -----------------------------------------------------------------------------


def test_the_designed_population_and_the_probe_bound_on_the_host():
    """The population of the device tests, checked where no device is needed, and the header's fp32 order over it against
    fp64 (ties aside), in units of 2^-24 of the scale: PROBE_BOUND is the next power of two at or above twice the largest."""
    st, _, pr, rec, groups = designed_population()
    check_population(st, rec, groups)
    ties = bodies_of(groups, "ties_0", "ties_c")
    worst = {"force": 0.0, "torque": 0.0, "tension": 0.0}
    for n in SIZES:
        r, s = record_for(rec, n), st[:n]
        off = ~np.isin(np.arange(n), ties)
        on = tr.taut_fp32(r, s)
        (got, got_T), ref, scale = tr.wrench_fp32_emulated(r, s, with_tension=True), tr.wrench(r, s, on), tr.wrench_scales(r, s, on)
        live = (tr.tension(r, s, on) > 0) & off
        assert not got[~live & off].any() and not got_T[~live & off].any()
        err = np.abs(got[live] - ref[live]) / (tr.ULP * scale[live])
        err_T = np.abs(got_T[live] - tr.tension(r, s, on)[live]) / (tr.ULP * tr.tension_scale(r, s, on)[live])
        worst = {"force": max(worst["force"], err[:, 0:3].max()), "torque": max(worst["torque"], err[:, 3:6].max()),
                 "tension": max(worst["tension"], err_T.max())}
    print("[tether, designed population, fp32 order emulated on the host] " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f" units of 2^-24 of the scale (bound {PROBE_BOUND:g})")
    largest = max(worst.values())
    assert largest <= PROBE_BOUND
    assert PROBE_BOUND == 2.0 ** np.ceil(np.log2(2.0 * largest))   # the rule: the next power of two at or above twice the largest


def test_the_header_s_fp32_order_is_exactly_antisymmetric():
    """F_i == -F_j and T_i == T_j, bit for bit, in the header's order carried out in fp32 - over the designed population (the
    ties, the clamped and the coincident pair included) and over random pairs."""
    st, _, _, rec, _ = designed_population()
    cases = [(record_for(rec, n), st[:n]) for n in SIZES]
    rs, rr = _random_pairs(600, 29)
    cases.append((rr.astype(np.float32), rs.astype(np.float32)))
    for r, s in cases:
        W, T = tr.wrench_fp32_emulated(r, s, with_tension=True)
        assert assert_antisymmetric(W, T, r) >= len(r) // 4


# ---- the physics -------------------------------------------------------------------------------------------------------------------------


def test_a_heavy_box_hangs_under_a_buoy_with_its_submerged_weight_on_the_line():
    """At rest the box is held by the line alone: its weight m g less its buoyancy rho V g (it is 5 m down, fully submerged:
    V = 0.5^3 = 0.125 m^3, 128.125 kg of water).  T = (200 - 128.125) * 9.81 = 705.09 N, whatever the line's stiffness."""
    st, pv, pr, sc, dt, weight = hanging_pair()
    k, c = Tether.for_pair(pr[0, 10], pr[1, 10], dt)
    lines = Tether([[0, 1]], length=LINE, stiffness=k, damping=c, n=2)
    lines.check_stable(pr[:, 10], dt)
    run = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 2400, teth=lines.record, implicit=True)
    s = run[-1]["state"].astype(np.float64)
    speed, T = np.linalg.norm(s[:, 7:10], axis=1), run[-1]["tether_tension"]
    print(f"[hanging pair] |v| {speed[0]:.2e}, {speed[1]:.2e} m/s  z {s[0, 2]:+.5f}, {s[1, 2]:+.5f} m  T {T[0]:.2f} N  (m - rho V) g {weight:.2f} N")
    assert weight == pytest.approx(705.09, abs=0.01)
    assert speed.max() < 1e-5
    assert T[0] == T[1] and abs(T[0] - weight) < 0.1
    assert s[0, 2] - s[1, 2] == pytest.approx(LINE + weight / k, abs=1e-3) and s[0, 2] < st[0, 2] - 0.05          # stretched by T / k; the buoy sits lower
    assert all(r["tether_taut"].all() for r in run[-600:])


def test_a_free_pair_keeps_its_momentum_to_the_rounding_of_the_additions():
    """No water, no gravity: the tether is the only force, F on one body and -F on the other - the SAME fp32 number, since the
    sum's rounding is symmetric.  In exact arithmetic m_a v_a + m_b v_b would not move at all; the integrator rounds each new
    velocity v + dt F / m to fp32 once, an error of at most half an ulp of the result, so per step the total momentum moves by
    at most sum_bodies m ulp(v') / 2 per axis - the bound formed here step by step - plus fp64 dust."""
    dt = float(np.float32(1.0 / 60.0))
    st, pv, pr = np.zeros((2, 13), np.float32), np.zeros((2, 6), np.float32), np.zeros((2, 11), np.float32)
    pr[:, 0:3], pr[:, 10] = (0.4, 0.5, 0.6), (3.0, 7.0)
    st[:, 6] = 1.0
    st[1, 0:3] = (2.0, 0.3, -0.1)
    st[0, 7:10], st[1, 7:10] = (-0.5, 0.1, 0.0), (0.7, -0.05, 0.2)
    st[0, 10:13] = (0.3, -0.2, 0.5)
    k, c = Tether.for_pair(3.0, 7.0, dt)
    l = float(np.linalg.norm(st[1, 0:3] + (0.0, 0.0, 0.25) - (0.15, 0.0, 0.0)))
    lines = Tether([[0, 1]], (0.15, 0.0, 0.0), (0.0, 0.0, 0.25), length=l - 0.2, stiffness=k, damping=c, n=2)
    run = closed_loop(st, pv, pr, 1025.0, 0.0, dt, 240, teth=lines.record, implicit=False, hydro=False)
    m = pr[:, 10].astype(np.float64)
    p0 = (m[:, None] * st[:, 7:10].astype(np.float64)).sum(axis=0)
    bound, p_before = np.zeros(3), p0
    pulled = 0
    for r in run:
        F = r["wrench"][:, 0:3]
        assert np.array_equal(F[0], -F[1])                         # equal and opposite, exactly
        pulled += bool(F.any())
        v = r["state"][:, 7:10]
        step_bound = (m[:, None] * 0.5 * np.spacing(np.abs(v)).astype(np.float64)).sum(axis=0) + 1e-13
        p = (m[:, None] * v.astype(np.float64)).sum(axis=0)
        assert (np.abs(p - p_before) <= step_bound).all(), (p - p_before, step_bound)      # this step's additions, and nothing else
        bound, p_before = bound + step_bound, p
        drift = np.abs(p - p0)
    dv = np.abs(run[-1]["state"][:, 7:10] - st[:, 7:10]).max()
    print(f"[free pair] the line pulled in {pulled} of 240 steps and changed a velocity by {dv:.3f} m/s; momentum drift {drift.max():.2e} kg m/s "
          f"within the additions' rounding {bound.max():.2e}")
    assert pulled > 20 and dv > 0.3 and drift.max() < 1e-4
