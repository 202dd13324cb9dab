"""Response statistics without a device (include/hydro.h, "Statistics"; silver2_isaacsim_amd/statistics.py): the header, the
binding and the record's layout; the marshalling of the two engine calls; ClosedLoopSim's bookkeeping with a recording engine;
`fold` - the header's arithmetic in NumPy - by hand on short sequences, on a sampled sinusoid whose statistics are known in
closed form, and against direct NumPy over the fp64 trajectory of config 1's buoy in a regular wave."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import statistics_reference as sx
from closed_loop_reference import closed_loop
from conftest import REPO
from mooring_population import buoy
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import simulate
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.sea import SeaSpectrum, SeaState
from silver2_isaacsim_amd.statistics import ResponseStatistics
from engine_stand_ins import ext_sim, ExtEngine, FUSED_HEAD, H, KE, make_engine, N, P13, refused, S, SO, STREAM, T, TILES, lib  # noqa: F401

ENTRIES = ("hydro_statistics_reset", "hydro_step_fused_tiled_multi_stat")
ENTRY = ENTRIES[1]
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
M3 = T((TILES, 27, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)
N2 = T((TILES, 14, 64), 0xC0000000)
PK = T((TILES, 2, 64), 0xC8000000)
ST = T((TILES, 11, 64), 0xD0000000)                               # the statistics record
LV = T((TILES, 2, 64), 0xD8000000)                                # its levels


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "added to 0.7.1 (no existing entry changed): hydro_statistics_reset, hydro_step_fused_tiled_multi_stat" in text.split("#define HYDRO_VERSION")[0]
    const = lambda name: int(re.search(r"#define " + name + r"\s+(\d+)", code).group(1))  # noqa: E731
    names = ("X", "Y", "Z", "VX", "VY", "VZ", "TENSION")
    assert [const("HYDRO_STAT_" + c) for c in names] == list(range(7)) == [getattr(nat, "STAT_" + c) for c in names] == [stx.INDEX[c.lower()] for c in names]
    assert const("HYDRO_STAT_CHANNELS") == nat.STAT_CHANNELS == len(stx.CHANNELS) == 7
    assert const("HYDRO_STAT_BYTES_PER_BODY") == nat.STAT_BYTES_PER_BODY == stx.BYTES_PER_BODY == 44 == 4 * 8 + 3 * 4
    assert const("HYDRO_STAT_TILE_BYTES") == 2816 == 64 * 44 == 4 * nat.STAT_FIELDS * 64 and const("HYDRO_STAT_LEVEL_FIELDS") == nat.STAT_LEVEL_FIELDS == 2
    # the _irr entry's signature with six arguments in front of step0
    irr, stat = nat.SIGNATURES["hydro_step_fused_tiled_multi_irr"], nat.SIGNATURES[ENTRY]
    six = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert stat[0] is irr[0] and stat[1] == irr[1][:-2] + six + irr[1][-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    head, tail = proto("hydro_step_fused_tiled_multi_irr").rsplit(" int64_t step0", 1)
    assert proto(ENTRY) == head + (" void *statistics, int64_t statistics_tile_stride, const float *levels, int64_t levels_tile_stride, "
                                   "int channel_a, int channel_b, int64_t step0") + tail
    for phrase in ("Statistics:", "mu + sigma * sqrt(2 ln N_up)", "EXACTLY the tension the extremes record samples", "THE LEVEL RECORD", "THE STATISTICS RECORD",
                   "READ AT THE START OF A LAUNCH AND\n * WRITTEN AT ITS END like the extremes", "NO fused multiply-add anywhere",
                   "the first sample never counts", "slack-to-taut events", "n is not touched inside the loop",
                   "A NaN sample makes that body's S1 and S2 of that slot NaN for good and nobody else's",
                   "NOT PROVIDED: heave relative to the moving surface; covariances between channels; more than two channels per record;",
                   "THE RECORD DOES NOT REMEMBER ITS CHANNELS", "statistics == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_irr",
                   "a replay accumulates and adds `steps` to n", "DESIGN.md section 30"):
        assert phrase in text, phrase
    assert 'means and variances' in text                         # the extremes' section still says what IT does not provide


def test_header_struct_is_plain_c(tmp_path):
    """The header with the record's struct through a C99 compiler at its strictest, and the layout the host assumes."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hydro.h"\n'
                   "int main(void) { hydro_statistics_tile_t t; t.words[2][63] = 0u;\n"
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof t, offsetof(hydro_statistics_tile_t, sums), offsetof(hydro_statistics_tile_t, words),\n'
                   "         sizeof t.sums[0], HYDRO_STAT_TILE_BYTES, HYDRO_STAT_BYTES_PER_BODY, HYDRO_STAT_TENSION);\n"
                   "  return (int)t.words[2][63]; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [2816, 0, 2048, 512, 2816, 44, 6]


def test_pack_and_unpack_follow_the_struct():
    n = 70
    rec = stx.empty(n)
    rec["sums"][:] = np.arange(n * 4, dtype=np.float64).reshape(n, 4) + 0.5
    rec["up"][:] = np.arange(n * 2, dtype=np.uint32).reshape(n, 2) | np.uint32(0x80000000)
    rec["n"][:] = 1000 + np.arange(n, dtype=np.uint32)
    tiled = stx.pack(rec)
    assert tiled.shape == (2, 11, 64) and tiled.dtype == np.float32
    raw = tiled.view(np.uint8).reshape(2, 2816)
    body = 65                                                     # tile 1, lane 1: sums[j][1] at 512 j + 8, words[w][1] at 2048 + 256 w + 4
    for j in range(4):
        assert raw[1, 512 * j + 8:512 * j + 16].view(np.float64)[0] == rec["sums"][body, j]
    assert raw[1, 2048 + 4:2048 + 8].view(np.uint32)[0] == rec["up"][body, 0] and raw[1, 2048 + 512 + 4:2048 + 512 + 8].view(np.uint32)[0] == rec["n"][body]
    assert sx.same_record(stx.unpack(tiled, n), rec, nan_equal=False)
    assert not raw[1, 512 * 0 + 8 * 6:512].any()                  # the padding lanes are zero


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_stat(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                                None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 1728, 3,
                                                None, 512, None, 896, 2, None, 128, None, 704, None, 128, 2, 6, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_statistics_reset(None, 64, None, 704, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


@pytest.fixture
def eng(lib):  # noqa: F811
    return make_engine(lib)


def test_statistics_reset(lib, eng):  # noqa: F811
    assert eng.statistics_reset(ST, N, stream=STREAM) is ST
    assert lib.calls == [("hydro_statistics_reset", (H, 1000, 0xD0000000, 704, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 11, 64) tensor on cuda:0", eng.statistics_reset, E, N, stream=STREAM)


def test_step_fused_tiled_multi_stat(lib, eng):  # noqa: F811
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    cases = [  # nothing at all: every record NULL with stride 0, the default channels z and tension
             (dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0, 1)
              + (None, 0) + (None, 0, 1) + (None, 0), (None, 0, None, 0, 2, 6), (0, STREAM)),
             (dict(statistics=ST, levels=LV, channel_a=5, channel_b=0, mooring=M3, mooring_layers=3, tether=N2, layers=2, peaks=PK, extremes=E, control=C,
                   applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + (0xA0000000, 1728, 3)
              + (0xA8000000, 512) + (0xC0000000, 896, 2) + (0xC8000000, 128), (0xD0000000, 704, 0xD8000000, 128, 5, 0), (123456789012, STREAM)),
             (dict(statistics=ST, levels=LV, extremes=E, applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0, 1) + (0xA8000000, 512)
              + (None, 0, 1) + (None, 0), (0xD0000000, 704, 0xD8000000, 128, 2, 6), (5, STREAM))]
    for kw, state_out, step0, head, six, tail in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_stat(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, head + six + tail)]
        # without the six arguments: argument for argument the _irr entry's call
        lib.calls.clear()
        kw2 = {k: v for k, v in kw.items() if k not in ("statistics", "levels", "channel_a", "channel_b")}
        eng.step_fused_tiled_multi_irr(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw2)
        assert lib.calls == [("hydro_step_fused_tiled_multi_irr", head + tail)]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 11, 64) tensor on cuda:0", eng.step_fused_tiled_multi_stat, S, P13, N, 0.01, 3, 0, E, LV, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 2, 64) tensor on cuda:0", eng.step_fused_tiled_multi_stat, S, P13, N, 0.01, 3, 0, ST, E, stream=STREAM)
    refused(lib, "mooring_layers must be in 1 .. 4", eng.step_fused_tiled_multi_stat, S, P13, N, 0.01, 3, 0, ST, LV, 2, 6, M3, 5, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class StatEngine(ExtEngine):
    """tests/engine_stand_ins.py's recording engine with the sea calls, the entries above the extremes and the two calls of the statistics."""

    def set_sea(self, sea):
        self.calls.append(("set_sea", sea))

    def set_sea_spectrum(self, spectrum):
        self.calls.append(("set_sea_spectrum", spectrum))

    def alloc_statistics(self, n):
        return self.alloc_tiled(11, n)

    def statistics_reset(self, statistics, n, stream=None):
        self.calls.append(("statistics_reset", statistics, n))
        return statistics

    def step_fused_tiled_multi_teth(self, cur, old, n, dt, steps, step0, tether, extremes, mooring, control, applied, frame, implicit_drag=False,
                                    ke_out=None, log=None, **rec):
        return self._step("teth", cur, steps, step0=step0, log=log)

    def step_fused_tiled_multi_net(self, cur, old, n, dt, steps, step0, tether, layers, extremes, mooring, control, applied, frame, implicit_drag=False,
                                   ke_out=None, log=None, **rec):
        return self._step("net", cur, steps, step0=step0, log=log)

    def step_fused_tiled_multi_peak(self, cur, old, n, dt, steps, step0, tether, layers, peaks, extremes, mooring, control, applied, frame,
                                    implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("peak", cur, steps, step0=step0, log=log)

    def step_fused_tiled_multi_spread(self, cur, old, n, dt, steps, step0, mooring, mooring_layers, tether, layers, peaks, extremes, control, applied,
                                      frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("spread", cur, steps, step0=step0, log=log)

    def step_fused_tiled_multi_irr(self, cur, old, n, dt, steps, step0, mooring, mooring_layers, tether, layers, peaks, extremes, control, applied,
                                   frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("irr", cur, steps, step0=step0, log=log)

    def step_fused_tiled_multi_stat(self, cur, old, n, dt, steps, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                    peaks, extremes, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("stat", cur, steps, step0=step0, statistics=statistics, levels=levels, channels=(channel_a, channel_b), mooring=mooring,
                          mooring_layers=mooring_layers, tether=tether, layers=layers, peaks=peaks, extremes=extremes, control=control, applied=applied,
                          frame=frame, log=log)


LINKS = dict(links=[[3, 4], [4, 5], [66, 69]], length=[5.0, 6.0, 8.0], stiffness=300.0, damping=25.0)
SPREAD = dict(anchors=[[[1.0, 2.0, -20.0], [-3.0, 4.0, -20.0], [5.0, -6.0, -20.0]], [[3.0, 4.0, -21.0], [7.0, 8.0, -21.0], [0.0, 0.0, 0.0]]],
              fairleads=(0.0, 0.1, -0.5), length=[[19.0, 20.0, 21.0], [20.0, 22.0, 0.0]], stiffness=[[2400.0, 2400.0, 2400.0], [3000.0, 3000.0, 0.0]],
              damping=200.0 * np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]]), bodies=[66, 3])
LINES = dict(anchor=[[1.0, 2.0, -20.0], [3.0, 4.0, -21.0]], fairlead=(0.0, 0.1, -0.5), length=[19.0, 20.0], stiffness=7200.0, damping=600.0, bodies=[66, 3])
#        recorder, applied, control, bed, spread, line, extremes, net, peaks, spectrum
COMBOS = {"plain": (False,) * 10, "rec": (True,) + (False,) * 9, "App": (False, True) + (False,) * 8, "Ctl": (False, False, True) + (False,) * 7,
          "Bed": (False,) * 3 + (True,) + (False,) * 6, "Spread": (False,) * 4 + (True,) + (False,) * 5, "Line": (False,) * 5 + (True,) + (False,) * 4,
          "Ext": (False,) * 6 + (True, False, False, False), "Net": (False,) * 7 + (True, False, False), "Peak": (False,) * 7 + (True, True, False),
          "Irr": (False,) * 9 + (True,), "all": (True,) * 5 + (False,) + (True,) * 4}
SPEC = SeaSpectrum((0.1, 0.0, 0.0)).add_wave(0.2, 0.06, 0.02, 0.8, 0.3)
STATE = np.zeros((70, 13), np.float32)
STATE[:, 2], STATE[:, 0] = -0.25 + 0.001 * np.arange(70), np.arange(70)


def _sim(monkeypatch, recorder=False, applied=False, control=False, bed=False, spread=False, line=False, extremes=False, net=False, peaks=False, spectrum=False):
    s = ext_sim(monkeypatch, recorder, applied, control, False, bed)
    s.engine = StatEngine()
    s.state = lambda: STATE
    if spread:
        s.set_mooring_spread(**SPREAD)
    if line:
        s.set_mooring(**LINES)
    if extremes:
        s.track_extremes()
    if net:
        s.set_tether_net(**LINKS)
    if peaks:
        s.track_link_tensions()
    if spectrum:
        s.set_sea(SPEC)
    s.engine.calls.clear()
    return s


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(COMBOS), ids=list(COMBOS))
def test_the_stat_entry_is_picked_with_every_runner_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, bed, spread, line, extremes, net, peaks, spectrum = COMBOS[combo]
    s = _sim(monkeypatch, *COMBOS[combo])
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert "stat" not in before and len(before) == 3
    s.engine.calls.clear()
    s.steps_done = 0
    s._graph = "a captured graph of another entry"
    view = s.track_statistics()
    assert view is s.statistics and isinstance(view, ResponseStatistics) and s._graph is None
    assert view.channels == ("z", "tension") and view.channel_numbers == (2, 6)
    assert np.array_equal(view.levels[:, 0], STATE[:, 2]) and not view.levels[:, 1].any()          # z from the current state, the tension against 0
    assert np.array_equal(view.levels_buffer.numpy()[1, 0, :6], STATE[64:70, 2]) and tuple(view.buffer.shape) == (2, 11, 64)
    assert s.engine.calls == [("statistics_reset", view.buffer, 70)]
    s.engine.calls.clear()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "stat" and call["steps"] == k and call["step0"] == done
        assert call["statistics"] is view.buffer and call["levels"] is view.levels_buffer and call["channels"] == (2, 6)
        assert call["mooring"] is (s.mooring_spread if spread else s.mooring) and call["mooring_layers"] == (3 if spread else 1)
        assert (call["mooring"] is not None) == (spread or line)
        assert call["extremes"] is (s.extremes.buffer if extremes else None)
        assert call["tether"] is s.tether_net and (s.tether_net is not None) == net and call["layers"] == (s.tether_layers if net else 1)
        assert call["peaks"] is (s.link_tensions.buffer if peaks else None)
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s._graph = "a captured graph of the statistics' entry"
    s.clear_statistics()
    assert s.statistics is None and s._graph is None and s.engine.calls == []
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.engine.calls.clear()
    s.clear_statistics()                                           # a second clear is nothing
    assert s.engine.calls == []


def test_a_change_of_channels_or_levels_needs_a_reset(monkeypatch):
    s = _sim(monkeypatch)
    view = s.track_statistics(("x", "vz"))
    assert view.channels == ("x", "vz") and np.array_equal(view.levels[:, 0], STATE[:, 0]) and not view.levels[:, 1].any()
    same = s.track_statistics(("z", "tension"))                    # nothing sampled yet: the record is empty, the channels may change
    assert same is view and same.buffer is view.buffer and same.levels_buffer is view.levels_buffer and view.channels == ("z", "tension")
    s.run_resident(2)
    s.engine.calls.clear()
    with pytest.raises(ValueError, match="reset=True"):
        s.track_statistics(("x", "tension"))
    with pytest.raises(ValueError, match="reset=True"):
        s.track_statistics(("z", "tension"), levels=(0.0, 1.0))
    assert s.engine.calls == [] and view.channels == ("z", "tension")
    assert s.track_statistics(("z", "tension")) is view and s.engine.calls == []                   # the same channels: it goes on accumulating
    s._graph = "captured"
    s.track_statistics(("x", "tension"), levels=(1.5, 0.0), reset=True)
    assert view.channels == ("x", "tension") and (view.levels == np.array([1.5, 0.0], np.float32)).all() and s._graph is None
    assert s.engine.calls == [("statistics_reset", view.buffer, 70)]
    s.run_resident(1)
    assert s.engine.calls[-1]["channels"] == (0, 6)
    view.reset()                                                   # the view's own reset also frees the channels
    s.track_statistics(("y", "vy"))
    assert view.channels == ("y", "vy")
    for bad in (("z",), ("z", "heave"), ("z", 7)):
        with pytest.raises(ValueError):
            s.track_statistics(bad, reset=True)
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.track_statistics()


def test_graph_replays_refuse_lines_and_waves_with_statistics_and_take_a_current(monkeypatch):
    s = _sim(monkeypatch)
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s.set_mooring(**LINES)
    s.set_sea(SeaState((0.3, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4))
    s.track_statistics()
    with pytest.raises(ValueError, match="cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [] and s.steps_done == 0


# ---- fold by hand -----------------------------------------------------------------------------------------------------------------
def _fold1(xs_a, xs_b, level_a, level_b, record=None):
    """fold for one body."""
    a, b = np.asarray(xs_a, np.float32)[:, None], np.asarray(xs_b, np.float32)[:, None]
    return stx.fold(record, a, b, np.array([[level_a, level_b]], np.float32))


def test_fold_by_hand():
    f = np.float32
    rec = _fold1([1.5, 0.25, 3.0], [0.0, 0.0, 0.0], 1.0, 0.0)
    d = [float(f(1.5)) - 1.0, float(f(0.25)) - 1.0, float(f(3.0)) - 1.0]
    assert rec["sums"][0, 0] == (d[0] + d[1]) + d[2] and rec["sums"][0, 1] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert rec["n"][0] == 3 and stx.upcrossings(rec, 0)[0] == 1 and rec["up"][0, 0] == 1           # above, below, above: one crossing, the last sample above
    assert not rec["sums"][0, 2:].any() and not np.signbit(rec["sums"][0, 2:]).any()
    assert rec["up"][0, 1] == 0x80000000                                                            # 0 is not above 0: never above, nothing counted
    # the first sample never counts, however high; x == L is not above
    assert stx.upcrossings(_fold1([9.0], [9.0], 1.0, 1.0), 0)[0] == 0
    assert stx.upcrossings(_fold1([0.0, 9.0], [1.0, 1.0], 1.0, 1.0), 0)[0] == 1
    rec = _fold1([1.0, 1.0, 1.0, 2.0], [0.5, 1.0, 0.5, 1.0], 1.0, 1.0)
    assert stx.upcrossings(rec, 0)[0] == 1 and stx.upcrossings(rec, 1)[0] == 0
    # L = 0 on a tension: slack-to-taut once per event, however long the line stays taut
    T = [0.0, 0.0, 5.0, 7.0, 6.0, 0.0, 0.0, 3.0, 0.0, 2.0, 2.5]
    rec = _fold1(T, T, 0.0, 0.0)
    assert stx.upcrossings(rec, 0)[0] == 3 and rec["sums"][0, 0] == sum(T) and rec["n"][0] == len(T)
    assert stx.upcrossings(_fold1(T[2:], T[2:], 0.0, 0.0), 0)[0] == 2                               # taut from the first sample: that one is no event
    # accumulation: two folds are one
    whole, first = _fold1(T, T[::-1], 1.0, 2.0), _fold1(T[:4], T[::-1][:4], 1.0, 2.0)
    assert sx.same_record(_fold1(T[4:], T[::-1][4:], 1.0, 2.0, first), whole, nan_equal=False)


def test_a_nan_sample_poisons_its_body_and_slot_only():
    a = np.array([[1.0, 1.0], [np.nan, 2.0], [3.0, 3.0]], np.float32)
    b = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]], np.float32)
    rec = stx.fold(None, a, b, np.zeros((2, 2), np.float32))
    assert np.isnan(rec["sums"][0, 0:2]).all() and np.isfinite(rec["sums"][0, 2:4]).all() and np.isfinite(rec["sums"][1]).all()
    assert rec["sums"][1, 0] == 6.0 and rec["sums"][0, 2] == 6.0 and (rec["n"] == 3).all()
    # the NaN is not above: 1 (above), NaN (not above), 3 (above): one crossing where the clean body has none
    assert stx.upcrossings(rec, 0).tolist() == [1, 0]
    assert np.isnan(stx.mean(rec, 0, np.zeros((2, 2), np.float32))[0]) and stx.mean(rec, 0, np.zeros((2, 2), np.float32))[1] == 2.0


def test_fold_refuses_what_it_cannot_fold():
    with pytest.raises(ValueError):
        stx.fold(None, np.zeros((3, 2)), np.zeros((3, 3)), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        stx.fold(None, np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((2, 3)))
    for bad in ("heave", 7, -1):
        with pytest.raises(ValueError):
            stx.channel_index(bad)


# ---- a sampled sinusoid -----------------------------------------------------------------------------------------------------------
class _HostSim:
    """What ResponseStatistics asks of a sim, over a host record."""
    n = 1

    def synchronize(self):
        pass


class _HostBuffer:
    def __init__(self, tiled):
        self._tiled = tiled

    def cpu(self):
        return self

    def numpy(self):
        return self._tiled


def test_a_sampled_sinusoid():
    """x_k = L + A sin(2 pi (k + 1/2) / P) in fp32, k = 0 .. M P - 1, P = 48 samples per period, M = 25 periods, about its level L.
    In exact arithmetic the samples of whole periods of a sinusoid at P > 2 equally spaced phases sum to 0 and their squares to
    A^2 / 2 each, so mean = L and std = A / sqrt(2) EXACTLY; the half-sample offset keeps every sample away from the level (the
    nearest is A sin(pi / 48) = 0.065 A), so each period crosses upwards once - at its start; the run starts above its level and the first
    sample never counts: M - 1 crossings; reversed in time the run starts below and every period counts: M.  What remains is rounding: each fp32 sample
    is off by at most 2^-24 (|L| + A) = 1.8e-7, so the mean by at most that and the variance by at most 2 A 1.8e-7 + (1.8e-7)^2;
    the fp64 sums add 1 200 terms with relative errors of 2^-53 each - eight orders below.  Bounds: 2e-7 on the mean, 1e-6
    relative on the standard deviation.  tz = M P dt / (M - 1): the duration over the crossings counted."""
    L, A, P, M, dt = 2.0, 1.0, 48, 25, 0.125
    k = np.arange(M * P)
    x = (L + A * np.sin(2.0 * math.pi * (k + 0.5) / P)).astype(np.float32)
    lev = np.array([[L, L]], np.float32)
    rec = stx.fold(None, x[:, None], x[::-1][:, None], lev)
    view = ResponseStatistics(_HostSim(), _HostBuffer(stx.pack(rec)), None, ("z", "vz"), lev)
    assert view.count()[0] == M * P
    for ch in ("z", "vz"):
        assert abs(view.mean(ch)[0] - L) <= 2e-7
        assert abs(view.std(ch)[0] / (A / math.sqrt(2.0)) - 1.0) <= 1e-6 and view.std(ch)[0] == math.sqrt(view.variance(ch)[0])
    assert view.upcrossings("z")[0] == M - 1                       # starts above: the first period's crossing is the first sample, which never counts
    assert view.upcrossings("vz")[0] == M                          # reversed in time it starts below: every period counts
    assert view.tz("z", dt)[0] == M * P * dt / (M - 1) and view.tz("vz", dt)[0] == P * dt
    mpm = view.most_probable_maximum("vz")[0]
    assert mpm == pytest.approx(L + A / math.sqrt(2.0) * math.sqrt(2.0 * math.log(M)), rel=1e-6)
    assert view.most_probable_maximum("vz", steps=4 * M * P)[0] == pytest.approx(L + A / math.sqrt(2.0) * math.sqrt(2.0 * math.log(4 * M)), rel=1e-6)
    with pytest.raises(ValueError, match="not tracked"):
        view.mean("x")


# ---- config 1's buoy in a regular wave ------------------------------------------------------------------------------------------
def test_fold_over_the_buoys_fp64_trajectory_is_numpys_mean_and_variance():
    """Config 1's buoy through closed_loop_reference.closed_loop in a regular wave, 600 steps: mean and variance from fold's sums
    against np.mean / np.var of the same fp32 samples in fp64.  Both sum 600 terms of magnitude <= D (the largest |d|) in fp64: the
    sums differ by at most 600 * 2^-52 * 600 D in the worst case, i.e. the means by 600 * 2^-52 D and the variances by
    2 * 600 * 2^-52 D^2 (plus the same again for the subtraction of the squared mean) - bounds 1e-12 D and 1e-12 D^2."""
    st, pv, pr, sc, dt, z_eq, _ = buoy()
    sea = SeaState((0.2, 0.0, 0.0)).add_wave(0.3, 2.0 * math.pi / 30.0, 0.0, math.sqrt(sc.g * 2.0 * math.pi / 30.0), 0.0)
    run = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 600, sea=sea, implicit=True)
    states = np.stack([np.asarray(r["state"], np.float32) for r in run])
    z, vz = states[:, :, 2], states[:, :, 9]
    lev = np.array([[z_eq, 0.0]], np.float32)
    rec = stx.fold(None, z, vz, lev)
    assert z.std() > 0.01                                          # the buoy heaves
    for slot, x in ((0, z), (1, vz)):
        x64 = x[:, 0].astype(np.float64)
        D = np.abs(x64 - float(lev[0, slot])).max()
        assert abs(stx.mean(rec, slot, lev)[0] - x64.mean()) <= 1e-12 * D
        assert abs(stx.variance(rec, slot)[0] - x64.var()) <= 1e-12 * D * D
    assert stx.upcrossings(rec, 0)[0] >= 2                         # 10 s in a wave of 4.4 s
    up, cnt = stx.upcrossings(rec, 0)[0], rec["n"][0]
    assert cnt == 600 and 2.0 <= cnt * dt / up <= 10.0


def test_the_crossing_scene_meets_its_requirement_on_the_reference_alone():
    """tests/test_statistics_gpu.py's wave of six steps: by the fp64 closed loop every copy's vz crosses its mean upwards, most of them more than once."""
    _, levels, rec = sx.crossing_reference(65)
    up = stx.upcrossings(rec, 0)
    assert (up > 0).mean() >= 0.25 and (up >= 2).any() and (rec["n"] == sx.CROSS_STEPS).all() and np.isfinite(levels).all()


# ---- the recorded figures ---------------------------------------------------------------------------------------------------------
def test_recorded_isa_figures_meet_the_lds_register_and_scratch_conditions():
    """profiles/statistics.json (scripts/diag_statistics.py --isa-only): each of the 2 x 32 instantiations keeps three blocks per CU
    (LDS <= 54 613 B: its family's plus 10 240), stays within 168 VGPRs and uses no scratch."""
    import json
    isa = json.load(open(os.path.join(REPO, "profiles", "statistics.json")))["isa"]
    per = isa["per_instantiation"]
    assert len(per) == 64 and isa["conditions_met"] is True
    for name, row in per.items():
        assert row["scratch_bytes"] == 0 and row["vgprs"] <= 168 and row["waves_per_simd"] >= 3, name
        assert row["lds_bytes"] == row["built_on_lds_bytes"] + 10240 <= 54613, name
    for family in isa["step_loop"].values():
        assert family["added"]["fp64"] == 8 and family["added"]["scratch"] == 0 and 0 < family["added"]["instructions"] <= 120
