"""The peak tension of every tether link (hydro_step_fused_tiled_multi_peak; silver2_isaacsim_amd.tether.LinkTensions) as far as a
machine without a GPU can see it: the C boundary, the Python host's marshalling (with the stand-ins of tests/engine_stand_ins.py),
ClosedLoopSim's bookkeeping with a fake engine under its three runners, the host restatement of the update against a brute-force
maximum, the view's `peak()` in the caller's order, and the precondition of tests/test_link_tensions_gpu.py: by the fp64 reference
(tests/link_tension_reference.py) the designed net's peaks fall on the first, on an interior and on the last of seven steps, in
layers 0 and 1, so that an implementation that keeps the first sample, the last sample or layer 0 only cannot pass there."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import link_tension_reference as ltr
import populations
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd.tether import LinkTensions
from engine_stand_ins import (BODIES, eng, ext_sim as _ext_sim, ExtEngine, FUSED_HEAD, KE, lib, LINES, N, P13, refused, S, SO, STREAM, T, TILES,
                              _without_extremes)  # noqa: F401  (fixtures are requested by name)
from tether_net_population import net_for, net_population, SIZES

ENTRY = "hydro_step_fused_tiled_multi_peak"
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
M = T((TILES, 9, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)
TT = T((TILES, 7, 64), 0xB0000000)                                # a net of one layer
N3 = T((TILES, 21, 64), 0xC0000000)                               # a net of three
P1 = T((TILES, 1, 64), 0xD0000000)                                # the record of one layer
P3 = T((TILES, 3, 64), 0xD8000000)                                # of three


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + ENTRY + r"\s*\(", code) and ENTRY in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "added to 0.7.1 (no existing entry changed): " + ENTRY in text.split("#define HYDRO_VERSION")[0]    # the version comment
    # the net entry's argument list with one pointer and one int64 between tether_layers and step0
    net, peak = (nat.SIGNATURES["hydro_step_fused_tiled_multi_" + k][1] for k in ("net", "peak"))
    assert peak == net[:-2] + [ctypes.c_void_p, ctypes.c_int64] + net[-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    tail = "int64_t step0, void *stream"
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_net")[:-len(tail)] + "float *tether_peaks, int64_t tether_peaks_tile_stride, " + tail
    for phrase in ("Link tensions:", "[tiles][L][64]", "row l\n * belongs to layer l", "tether_peaks_tile_stride >= 64 L", "T where the line pulls, +0\n * where it adds nothing",
                   "exactly the value hydro_tether_wrench writes to\n * its `tension` output", "A NaN sample never enters, a NaN in the\n * record stays",
                   "an equal value leaves the record's bits", "ACCUMULATES over launches, chunks and graph replays", "a plain zero fill resets it",
                   "The padding lanes of the last tile", "never written", "NOTHING FEEDS BACK", "tension_max of the extremes record stays the mooring line's",
                   "tether_peaks == NULL : the launch and its bits are those of hydro_step_fused_tiled_multi_net", "a record with tether == NULL",
                   "safe to capture"):
        assert phrase in text, phrase


def test_library_exports_the_entry(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + ENTRY + r"$", out, re.M) and hasattr(nat.load(), ENTRY)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    written = ctypes.c_int64(-7)
    rc = nat.load().hydro_step_fused_tiled_multi_peak(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                                      None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 576,
                                                      None, 512, None, 896, 2, None, 128, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_step_fused_tiled_multi_peak(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    line, record = (0xA0000000, 576), (0xA8000000, 512)
    cases = [(TT, 1, P1, dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0) + (None, 0)
              + (0xB0000000, 448, 1) + (0xD0000000, 64) + (0, STREAM)),
             # three layers: the record's stride is 3 * 64, and it stands between `layers` and step0
             (N3, 3, P3, dict(extremes=E, mooring=M, control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + line + record
              + (0xC0000000, 1344, 3) + (0xD8000000, 192) + (123456789012, STREAM)),
             (N3, 3, P3, dict(extremes=E, applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0) + record + (0xC0000000, 1344, 3)
              + (0xD8000000, 192) + (5, STREAM)),
             # no record: NULL and stride 0 - the library dispatches to the net entry's launch
             (N3, 3, None, dict(mooring=M, control=C), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, 0x90000000, 1088) + line + (None, 0) + (0xC0000000, 1344, 3)
              + (None, 0) + (9, STREAM)),
             # neither a net nor a record
             (None, 2, None, dict(), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0) + (None, 0) + (None, 0, 2) + (None, 0) + (9, STREAM))]
    for net, layers, peaks, kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_peak(S, P13, N, 0.01, 7, step0, net, layers, peaks, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, want)]
    lib.calls.clear()
    # the record has one row per layer of the net
    refused(lib, "expected contiguous float32 (>= 16, 3, 64) tensor on cuda:0", eng.step_fused_tiled_multi_peak, S, P13, N, 0.01, 3, 0, N3, 3, P1, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 1, 64) tensor on cuda:0", eng.step_fused_tiled_multi_peak, S, P13, N, 0.01, 3, 0, TT, 1, P3, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 21, 64) tensor on cuda:0", eng.step_fused_tiled_multi_peak, S, P13, N, 0.01, 3, 0, TT, 3, P3, stream=STREAM)
    for layers in (0, 5, -1):
        refused(lib, "layers must be in 1 .. 4", eng.step_fused_tiled_multi_peak, S, P13, N, 0.01, 3, 0, N3, layers, P3, stream=STREAM)
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_peak, S, P13, N, 0.01, 3, 0, N3, 3, P3, E, M, C, A, "local", stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class PeakEngine(ExtEngine):
    """tests/engine_stand_ins.py's recording engine with the tether call, the net call and the call of the link tensions."""

    def step_fused_tiled_multi_teth(self, cur, old, n, dt, steps, step0, tether, extremes, mooring, control, applied, frame, implicit_drag=False,
                                    ke_out=None, log=None, **rec):
        return self._step("teth", cur, steps, step0=step0, tether=tether, extremes=extremes, mooring=mooring, control=control, applied=applied,
                          frame=frame, log=log)

    def step_fused_tiled_multi_net(self, cur, old, n, dt, steps, step0, tether, layers, extremes, mooring, control, applied, frame, implicit_drag=False,
                                   ke_out=None, log=None, **rec):
        return self._step("net", cur, steps, step0=step0, tether=tether, layers=layers, extremes=extremes, mooring=mooring, control=control,
                          applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_peak(self, cur, old, n, dt, steps, step0, tether, layers, peaks, extremes, mooring, control, applied, frame,
                                    implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("peak", cur, steps, step0=step0, tether=tether, layers=layers, peaks=peaks, extremes=extremes, mooring=mooring,
                          control=control, applied=applied, frame=frame, log=log)


def _sim(monkeypatch, recorder=False, applied=False, control=False, sea=False, bed=False, lines=False, extremes=False):
    s = _ext_sim(monkeypatch, recorder, applied, control, sea, bed)
    s.engine = PeakEngine()
    if lines:
        s.set_mooring(**LINES)
    if extremes:
        s.track_extremes()
        s.engine.calls.clear()
    return s


# the chain 3 - 4 - 5 - 6 of tile 0, a bridle between 66 and 69 and a third line at 66: three layers (tests/test_tether_net.py's)
LINKS = dict(links=[[3, 4], [4, 5], [5, 6], [66, 69], [66, 69], [66, 70 - 3]], fairlead_a=(0.0, 0.1, -0.5), fairlead_b=(0.0, 0.0, 0.25),
             length=[5.0, 6.0, 7.0, 8.0, 9.0, 10.0], stiffness=300.0, damping=25.0)
PAIRS = dict(pairs=[[66, 69], [3, 40]], length=5.0, stiffness=1800.0, damping=150.0)
COMBOS = {"plain": (False,) * 7, "rec": (True,) + (False,) * 6, "Ext": (False,) * 6 + (True,), "all": (True,) * 7}


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("tethers", ["net", "set_tether"])
@pytest.mark.parametrize("combo", list(COMBOS), ids=list(COMBOS))
def test_the_entry_is_picked_with_every_runner_and_cleared_again(monkeypatch, combo, tethers, run):
    recorder, applied, control, sea, bed, lines, extremes = COMBOS[combo]
    s = _sim(monkeypatch, *COMBOS[combo])
    assert simulate.ClosedLoopSim.link_tensions is None and s.link_tensions is None
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    if tethers == "net":
        buf, layers, parent = s.set_tether_net(**LINKS), 3, "net"
    else:
        buf, layers, parent = s.set_tether(**PAIRS), 1, "teth"
    go()
    before = [c["method"] for c in s.engine.calls]
    assert before == [parent] * 3
    s.engine.calls.clear()
    s.steps_done = 0
    view = s.track_link_tensions()
    assert view is s.link_tensions and isinstance(view, LinkTensions) and tuple(view.buffer.shape) == (2, layers, 64) and view.layers == layers
    assert s.engine.calls == [] and not view.buffer.any()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        # with a net: its buffer and its layers; with set_tether's record: that record as a net of one layer
        assert call["method"] == "peak" and call["steps"] == k and call["step0"] == done and call["tether"] is buf and call["layers"] == layers
        assert call["peaks"] is view.buffer
        assert call["extremes"] is (s.extremes.buffer if extremes else None)
        assert call["mooring"] is s.mooring and (s.mooring is not None) == lines
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    view.buffer[0, 0, 3] = 7.0
    s.clear_link_tensions()
    assert s.link_tensions is None and s.engine.calls == [] and view.buffer[0, 0, 3] == 7.0       # the record keeps its contents
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.clear_link_tensions()                                        # a second clear is nothing
    assert len(s.engine.calls) == 3
    again = s.track_link_tensions()
    assert again is view and not view.buffer.any()                 # the same buffer, reset


def test_track_link_tensions_needs_tethers_and_the_layer_count_is_fixed_while_tracking(monkeypatch):
    s = _sim(monkeypatch)
    with pytest.raises(ValueError, match=r"no tethers to track: call set_tether_net\(\) or set_tether\(\) first"):
        s.track_link_tensions()
    assert s.link_tensions is None
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.track_link_tensions()
    s.fused = True
    net = s.set_tether_net(**LINKS)
    view = s.track_link_tensions()
    assert view.layers == 3 and view.links.tolist() == LINKS["links"] and view.layer.tolist() == [0, 1, 0, 0, 1, 2]
    # another number of layers, or no tethers at all, under the record: refused, and nothing has changed
    two = {**LINKS, "links": LINKS["links"][:3], "length": LINKS["length"][:3]}
    for change in (lambda: s.set_tether_net(**two), s.clear_tether_net):
        with pytest.raises(ValueError, match=r"tracked over 3 layer\(s\): clear_link_tensions\(\) first"):
            change()
        assert s.tether_net is net and s.tether_layers == 3 and s.link_tensions is view
    # the same number of layers: the record stays, peak() reads the new links
    view.buffer[1, 2, 2] = 5.0
    s.set_tether_net(**{**LINKS, "links": LINKS["links"][::-1]})
    assert view.buffer[1, 2, 2] == 5.0 and view.links.tolist() == LINKS["links"][::-1] and view.layers == 3
    s.clear_link_tensions()
    s.set_tether_net(**two)
    assert s.track_link_tensions().layers == 2 and s.link_tensions is not view
    s.clear_link_tensions()
    s.clear_tether_net()
    s.set_tether(**PAIRS)
    one = s.track_link_tensions()
    assert one.layers == 1 and one.links.tolist() == PAIRS["pairs"] and one.layer.tolist() == [0, 0]
    with pytest.raises(ValueError, match=r"clear_link_tensions\(\) first"):
        s.clear_tether()
    assert s.tether is not None
    s.set_tether(**PAIRS)                                          # new contents under one layer: allowed
    assert s.link_tensions is one


def test_tracking_invalidates_a_captured_graph_only_when_it_changes_the_entry(monkeypatch):
    s = _sim(monkeypatch, lines=True)
    s.set_tether_net(**LINKS)
    s._graph = "a captured graph of the net entry"
    view = s.track_link_tensions()
    assert s._graph is None                                      # captured launches are of another entry
    s._graph = "a captured graph with the record"
    assert s.track_link_tensions() is view
    assert s._graph == "a captured graph with the record"       # a reset: the same entry, the same buffers
    s.clear_link_tensions()
    assert s._graph is None
    s._graph = "a captured graph of the net entry"
    s.clear_link_tensions()                                      # nothing to clear: the capture stands
    assert s._graph == "a captured graph of the net entry"


# ---- the view ----------------------------------------------------------------------------------------------------------------------
def test_fold_is_the_compare_and_select_maximum():
    rng = np.random.default_rng(7)
    rows, L, n = 9, 3, 130
    T = rng.uniform(0.0, 50.0, (rows, L, n)).astype(np.float32)
    T[rng.random(T.shape) < 0.4] = 0.0                           # a line that adds nothing: +0
    T[2, 1, 5] = T[0, 0, 9] = T[8, 2, 64] = np.nan               # NaN samples: first, interior and last
    T[:, 2, 100] = np.nan                                        # nothing but NaN samples
    T[:, 0, 77] = 0.0                                            # a line that never pulls
    got = LinkTensions.fold(T)
    assert got.shape == (n, L) and got.dtype == np.float32
    brute = np.zeros((n, L), np.float32)
    for i in range(n):
        for l in range(L):
            for r in range(rows):
                if T[r, l, i] > brute[i, l]:
                    brute[i, l] = T[r, l, i]
    assert np.array_equal(got.view(np.uint32), brute.view(np.uint32))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got, np.nan_to_num(T, nan=0.0).max(axis=0).T)       # a NaN sample never enters
    assert got[100, 2] == 0.0 and got[77, 0] == 0.0 and not np.signbit(got).any() and (got > 0).mean() > 0.9
    # a seed: a huge value and a NaN stay, +0 takes the largest sample, an equal value leaves the seed
    seed = np.zeros((n, L), np.float32)
    seed[3, 0], seed[4, 1], seed[6, 2] = 1e30, np.nan, got[6, 2]
    seeded = LinkTensions.fold(T, seed)
    assert seeded[3, 0] == np.float32(1e30) and np.isnan(seeded[4, 1]) and seeded[6, 2] == got[6, 2]
    rest = np.ones((n, L), bool)
    rest[3, 0] = rest[4, 1] = False
    assert np.array_equal(seeded[rest].view(np.uint32), got[rest].view(np.uint32)) and not seed[5].any()
    # the fold of two halves, the second seeded with the first, is the fold of the whole: the record accumulates
    assert np.array_equal(LinkTensions.fold(T[4:], LinkTensions.fold(T[:4])).view(np.uint32), got.view(np.uint32))
    for bad in (T[0], T[:, :, :5].reshape(-1)):
        with pytest.raises(ValueError, match=r"\(rows, L, n\)"):
            LinkTensions.fold(bad)
    with pytest.raises(ValueError, match=r"seed must be \(130, 3\)"):
        LinkTensions.fold(T, seed.T)
    # link_tension_reference.fold is the same rule in fp64, and names the step
    peak, when = ltr.fold(T)
    assert np.array_equal(peak.T.astype(np.float32), got) and when[2, 100] == -1 and when[0, 77] == -1
    i, l = np.argwhere(got > 0)[0]
    assert T[when[l, i], l, i] == got[i, l]


def test_peak_reads_each_link_at_its_first_body_in_its_layer_in_the_callers_order(monkeypatch):
    s = _sim(monkeypatch)
    s.set_tether_net(**LINKS)
    view = s.track_link_tensions()
    rec = np.zeros((BODIES, 3), np.float32)
    # both ends of a link hold its value, in the link's layer (greedy layers 0, 1, 0 | 0, 1, 2)
    for value, ((a, b), l) in enumerate(zip(LINKS["links"], [0, 1, 0, 0, 1, 2]), start=1):
        rec[a, l] = rec[b, l] = 10.0 * value
    view.buffer.copy_(simulate.torch.from_numpy(scenes.to_tiled(rec)))
    assert np.array_equal(view.record(), rec) and view.record().shape == (BODIES, 3)
    assert view.peak().tolist() == [10.0, 20.0, 30.0, 40.0, 50.0, 60.0]
    s.set_tether_net(**{**LINKS, "links": LINKS["links"][::-1], "length": LINKS["length"][::-1]})          # another order, other layers: 66's lines first
    assert view.layer.tolist() == [0, 1, 2, 0, 1, 0]
    assert view.peak(rec).tolist() == [rec[66, 0], rec[66, 1], rec[66, 2], rec[5, 0], rec[4, 1], rec[3, 0]]
    view.reset()
    assert not view.buffer.any() and not view.peak().any()


# ---- the precondition of the device test -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_the_designed_nets_peaks_fall_on_first_interior_and_last_steps_in_two_layers(implicit):
    """Seven steps of the designed net by the fp64 reference: layers 0 and 1 each have at least 16 bodies whose peak is the first
    step's sample, at least 28 an interior step's and at least 2 the last step's; layer 2 has exactly two bodies with a peak,
    layer 3 none."""
    st, pv, pr, net, _ = net_population()
    for n in SIZES:
        with np.errstate(all="ignore"):                          # (explicit steps carry light bodies out of range)
            peak, when, rows = ltr.closed_loop_peaks(st[:n], pv[:n], pr[:n], populations.RHO, populations.G, populations.DT, 7, net=net_for(net, n),
                                                     implicit=implicit)
        assert peak.shape == when.shape == (4, n) and len(rows) == 7
        for l in (0, 1):
            first, interior, last = (when[l] == 0).sum(), ((when[l] > 0) & (when[l] < 6)).sum(), (when[l] == 6).sum()
            print(f"[link tensions, fp64 reference, n = {n}, {'implicit' if implicit else 'explicit'}, layer {l}] peak on the first step {first}, "
                  f"an interior step {interior}, the last step {last}")
            assert first >= 16 and interior >= 28 and last >= 2, (n, l, first, interior, last)
        assert (peak[2] > 0).sum() == 2 and not (peak[3] > 0).any() and not peak[3].any()
        # both ends of a link: the same peak
        for l in range(4):
            j = 64 * (np.arange(n) // 64) + net_for(net, n)[:, 7 * l + 6].astype(np.int64)
            assert np.array_equal(peak[l], peak[l][j], equal_nan=True), (n, l)
