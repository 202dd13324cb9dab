"""Tether nets (hydro_step_fused_tiled_multi_net; silver2_isaacsim_amd.tether.TetherNet) as far as a machine without a GPU can
see them: the C boundary, the Python host's marshalling (with the stand-ins of tests/engine_stand_ins.py), ClosedLoopSim's
bookkeeping with a fake engine under its three runners, every refusal of TetherNet and set_tether_net, the layering, the host
restatement against the fp64 reference of tests/tether_net_reference.py, the designed net of tests/test_tether_net_gpu.py, and
two physical cases through closed_loop_reference.closed_loop (wrapped by tether_net_reference.closed_loop_net).

THE FIGURES of the physical cases (dt = 1/60):
  a free chain (no water, no gravity) of 2, 5, 3 and 9 kg with offset fairleads, its ends parting: over 240 steps the total
      momentum moves by no more than the rounding of the velocity additions and of each body's summed wrench, the bound the
      test forms step by step
  the hanging chain (tether_net_population.hanging_chain: config 1's buoy, four 0.25 m, 25 kg boxes on 1.25 m links; implicit
      drag, water of 1025 kg/m^3), uniform constants at HALF the per-body stability bound (k = 450.0 N/m, c = 7.5 N s/m: five
      times and once TetherNet.for_chain's): each link carries the submerged weight below it, 352.55, 264.41, 176.27 and
      88.14 N.  The fp64 run of this scene shows after 3600 steps |T - weight| <= 0.0362 N and |v| <= 2.02e-4 m/s (the buoy's
      slow heave decays last); the thresholds are twice those figures, 0.0724 N and 4.04e-4 m/s, here and on the device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tether_net_reference as tnr
import tether_reference as tr
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd import tether as th
from silver2_isaacsim_amd.mooring import DEFAULT_C, DEFAULT_K, STABLE
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.tether import Tether, TetherNet
from engine_stand_ins import (BODIES, eng, ext_sim as _ext_sim, ExtEngine, FUSED_HEAD, H, KE, lib, LINES, N, P13, refused, S, SO, STREAM, T, TILES,
                              _without_extremes)  # noqa: F401  (fixtures are requested by name)
from tether_net_population import check_net, hanging_chain, hanging_constants, HANG_SPEED, HANG_STEPS, HANG_TENSION, LINK, net_population

ENTRY = "hydro_step_fused_tiled_multi_net"
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
M = T((TILES, 9, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)
TT = T((TILES, 7, 64), 0xB0000000)                                # a net of one layer
N3 = T((TILES, 21, 64), 0xC0000000)                               # a net of three


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + ENTRY + r"\s*\(", code) and ENTRY in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "hydro_step_fused_tiled_multi_net, HYDRO_TETH_LAYERS_MAX" in text.split("#define HYDRO_VERSION")[0]    # the version comment
    assert int(re.search(r"#define HYDRO_TETH_LAYERS_MAX\s+(\d+)", code).group(1)) == nat.TETH_LAYERS_MAX == th.LAYERS_MAX == tnr.LAYERS_MAX == 4
    # the tether entry's argument list with one int64, `tether_layers`, between tether_tile_stride and step0
    teth, net = (nat.SIGNATURES["hydro_step_fused_tiled_multi_" + k][1] for k in ("teth", "net"))
    assert net == teth[:-2] + [ctypes.c_int64] + teth[-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    tail = "int64_t step0, void *stream"
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_teth")[:-len(tail)] + "int64_t tether_layers, " + tail
    for phrase in ("Tether net:", "1 <= L <= HYDRO_TETH_LAYERS_MAX = 4", "[tiles][7 L][64]", "row 7 l + f", "tether_tile_stride >= 448 L",
                   "EACH LAYER IS A COMPLETE, VALID TETHER RECORD", "`tether + 448 l` with the net's tile\n * stride is an argument for hydro_tether_wrench",
                   "IN\n * ASCENDING LAYER ORDER", "+0 is not added", "every line lies inside one tile of 64 bodies", "at most 64\n * bodies",
                   "at most 4 lines per body", "the tether tensions still do not enter the extremes record", "tether_layers is ignored",
                   "tether_layers == 1  : the bits of hydro_step_fused_tiled_multi_teth", "2 (sum of k over the body's lines) dt^2 / m_i <= 0.04"):
        assert phrase in text, phrase


def test_library_exports_the_entry(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + ENTRY + r"$", out, re.M) and hasattr(nat.load(), ENTRY)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    written = ctypes.c_int64(-7)
    rc = nat.load().hydro_step_fused_tiled_multi_net(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                                     None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 576,
                                                     None, 512, None, 896, 2, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_step_fused_tiled_multi_net(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    line, record = (0xA0000000, 576), (0xA8000000, 512)
    cases = [(TT, 1, dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0) + (None, 0)
              + (0xB0000000, 448, 1) + (0, STREAM)),
             # three layers: the stride is 7 * 3 * 64, and `layers` stands between it and step0
             (N3, 3, dict(extremes=E, mooring=M, control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + line + record
              + (0xC0000000, 1344, 3) + (123456789012, STREAM)),
             (N3, 3, dict(extremes=E, applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0) + record + (0xC0000000, 1344, 3)
              + (5, STREAM)),
             # no net: NULL and stride 0 (the library dispatches to the extremes entry's launch); `layers` travels as given
             (None, 2, dict(mooring=M, control=C), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, 0x90000000, 1088) + line + (None, 0) + (None, 0, 2) + (9, STREAM))]
    for net, layers, kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_net(S, P13, N, 0.01, 7, step0, net, layers, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_net, S, P13, N, 0.01, 3, 0, N3, 3, E, M, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 14, 64) tensor on cuda:0", eng.step_fused_tiled_multi_net, S, P13, N, 0.01, 3, 0, N3, 2, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 21, 64) tensor on cuda:0", eng.step_fused_tiled_multi_net, S, P13, N, 0.01, 3, 0, TT, 3, stream=STREAM)
    for layers in (0, 5, -1):
        refused(lib, "layers must be in 1 .. 4", eng.step_fused_tiled_multi_net, S, P13, N, 0.01, 3, 0, N3, layers, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 8, 64) tensor on cuda:0", eng.step_fused_tiled_multi_net, S, P13, N, 0.01, 3, 0, N3, 3, M, stream=STREAM)


def test_tether_net_wrench_probes_each_layer_on_its_sub_record(lib, eng, monkeypatch):
    made = []

    def alloc(fields, n):
        made.append(T((TILES, fields, 64), 0xD0000000 + 0x1000000 * len(made)))
        return made[-1]
    monkeypatch.setattr(eng, "alloc_tiled", alloc)
    wrenches, tensions = eng.tether_net_wrench(S, N3, N, 3, stream=STREAM)
    assert [w.shape for w in wrenches] == [(TILES, 6, 64)] * 3 and [t.shape for t in tensions] == [(TILES, 1, 64)] * 3
    # layer l: the net's address + 448 l floats, the net's stride
    assert lib.calls == [("hydro_tether_wrench", (H, 1000, 0x10000000, 832, 0xC0000000 + 4 * 448 * l, 1344, 0xD0000000 + 0x2000000 * l, 384,
                                                  0xD1000000 + 0x2000000 * l, 64, STREAM)) for l in range(3)]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 14, 64) tensor on cuda:0", eng.tether_net_wrench, S, N3, N, 2, stream=STREAM)
    refused(lib, "layers must be in 1 .. 4", eng.tether_net_wrench, S, N3, N, 0, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class NetEngine(ExtEngine):
    """tests/engine_stand_ins.py's recording engine with the tether call and the net call."""

    def step_fused_tiled_multi_teth(self, cur, old, n, dt, steps, step0, tether, extremes, mooring, control, applied, frame, implicit_drag=False,
                                    ke_out=None, log=None, **rec):
        return self._step("teth", cur, steps, step0=step0, tether=tether, extremes=extremes, mooring=mooring, control=control, applied=applied,
                          frame=frame, log=log)

    def step_fused_tiled_multi_net(self, cur, old, n, dt, steps, step0, tether, layers, extremes, mooring, control, applied, frame, implicit_drag=False,
                                   ke_out=None, log=None, **rec):
        return self._step("net", cur, steps, step0=step0, tether=tether, layers=layers, extremes=extremes, mooring=mooring, control=control,
                          applied=applied, frame=frame, log=log)


def _sim(monkeypatch, recorder=False, applied=False, control=False, sea=False, bed=False, lines=False, extremes=False):
    s = _ext_sim(monkeypatch, recorder, applied, control, sea, bed)
    s.engine = NetEngine()
    if lines:
        s.set_mooring(**LINES)
    if extremes:
        s.track_extremes()
        s.engine.calls.clear()
    return s


# the chain 3 - 4 - 5 - 6 of tile 0, a bridle between 66 and 69 and a third line at 66: three layers
LINKS = dict(links=[[3, 4], [4, 5], [5, 6], [66, 69], [66, 69], [66, 70 - 3]], fairlead_a=(0.0, 0.1, -0.5), fairlead_b=(0.0, 0.0, 0.25),
             length=[5.0, 6.0, 7.0, 8.0, 9.0, 10.0], stiffness=300.0, damping=25.0)
COMBOS = {"plain": (False,) * 7, "rec": (True,) + (False,) * 6, "App": (False, True) + (False,) * 5, "Sea": (False, False, False, True, False, False, False),
          "Moor": (False,) * 5 + (True, False), "Ext": (False,) * 6 + (True,), "all": (True,) * 7}


def _without_net(recorder, applied, control, sea, bed, lines, extremes, eager):
    return "ext" if extremes else _without_extremes(recorder, applied, control, sea, bed, lines, eager)


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(COMBOS), ids=list(COMBOS))
def test_the_net_entry_is_picked_with_every_runner_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, sea, bed, lines, extremes = COMBOS[combo]
    s = _sim(monkeypatch, *COMBOS[combo])
    assert simulate.ClosedLoopSim.tether_net is None and s.tether_net is None and s.tether_layers == 0
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert before == [_without_net(*COMBOS[combo], eager=run != "resident")] * 3
    s.engine.calls.clear()
    s.steps_done = 0
    buf = s.set_tether_net(**LINKS)
    assert buf is s.tether_net and s.tether_layers == 3 and tuple(buf.shape) == (2, 21, 64) and s.engine.calls == []
    # the record: layer l in fields 7 l .. 7 l + 6; greedy layers 0, 1, 0 for the chain and 0, 1, 2 at body 66
    rows = scenes.from_tiled(buf.numpy(), BODIES)
    assert rows[4, 0:7].tolist() == [0.0, 0.0, 0.25, 5.0, 300.0, 25.0, 3.0] and rows[4, 7:14].tolist() == [0.0, np.float32(0.1), -0.5, 6.0, 300.0, 25.0, 5.0]
    assert rows[5, 0:7].tolist() == [0.0, np.float32(0.1), -0.5, 7.0, 300.0, 25.0, 6.0] and rows[5, 7:14].tolist() == [0.0, 0.0, 0.25, 6.0, 300.0, 25.0, 4.0]
    assert rows[66, 3::7].tolist() == [8.0, 9.0, 10.0] and rows[66, 6::7].tolist() == [5.0, 5.0, 3.0] and rows[67, 14:21].tolist() == [0.0, 0.0, 0.25, 10.0, 300.0, 25.0, 2.0]
    others = np.delete(np.arange(BODIES), [3, 4, 5, 6, 66, 67, 69])
    assert not rows[others][:, [f for f in range(21) if f % 7 != 6]].any() and (rows[others, 6::7] == (others % 64)[:, None]).all()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "net" and call["steps"] == k and call["step0"] == done and call["tether"] is buf and call["layers"] == 3
        assert call["extremes"] is (s.extremes.buffer if extremes else None)
        assert call["mooring"] is s.mooring and (s.mooring is not None) == lines
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the net was set)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_tether_net()
    assert s.tether_net is None and s.tether_layers == 0 and s.engine.calls == []
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.clear_tether_net()                                           # a second clear is nothing
    assert len(s.engine.calls) == 3
    assert s.set_tether_net(**LINKS) is buf                        # the buffer's address does not change


def test_a_net_and_a_tether_record_exclude_each_other(monkeypatch):
    pairs = dict(pairs=[[66, 69], [3, 40]], length=5.0, stiffness=1800.0, damping=150.0)
    s = _sim(monkeypatch)
    s.set_tether(**pairs)
    with pytest.raises(ValueError, match=r"clear_tether\(\) first"):
        s.set_tether_net(**LINKS)
    assert s.tether_net is None and s.tether is not None
    s.run_resident(2)
    assert [c["method"] for c in s.engine.calls] == ["teth"]         # set_tether keeps its own entry
    s.clear_tether()
    s.set_tether_net(**LINKS)
    with pytest.raises(ValueError, match=r"clear_tether_net\(\) first"):
        s.set_tether(**pairs)
    assert s.tether is None and s.tether_net is not None
    s.clear_tether_net()
    s.set_tether(**pairs)
    s.engine.calls.clear()
    s.run_resident(2)
    assert [c["method"] for c in s.engine.calls] == ["teth"]


def test_graph_replays_take_a_net_and_a_current_and_refuse_waves(monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s = _sim(monkeypatch, lines=True)
    s._graph = "a captured graph without a net"
    s.set_tether_net(**LINKS)
    assert s._graph is None                                      # captured launches are of another entry
    s._graph = "a captured graph with the net"
    s.set_tether_net(**LINKS)
    assert s._graph == "a captured graph with the net"          # new contents, the same entry, buffer and layers: the capture stands
    s.set_tether_net(**{**LINKS, "links": LINKS["links"][:3], "length": LINKS["length"][:3]})
    assert s._graph is None and s.tether_layers == 2            # another number of layers: another buffer, another argument
    s.sea = SeaState((0.3, 0.0, 0.0))
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]
    s.sea = SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [32] and s.steps_done == 0
    s._graph = "a captured graph with the net"
    s.clear_tether_net()
    assert s._graph is None


def test_set_tether_net_refusals(monkeypatch):
    s = _sim(monkeypatch)
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_tether_net(**LINKS)
    s.fused = True
    with pytest.raises(ValueError, match="outside 0 .. 69"):
        s.set_tether_net(**{**LINKS, "links": [[66, 70]], "length": 5.0})
    with pytest.raises(ValueError, match="tiles 0 and 1.*inside one block of 64"):
        s.set_tether_net(**{**LINKS, "links": [[3, 4], [4, 64]], "length": 5.0})
    with pytest.raises(ValueError, match=">= 0"):
        s.set_tether_net(**{**LINKS, "damping": -1.0})
    # the per-body rule for the bodies' masses (500 kg): body 66 carries three lines, 2 * 3 k dt^2 / m
    with pytest.raises(ValueError, match=r"body 66 \(3 lines\) has 2 sum\(k\) dt\^2 / m = 0.048"):
        s.set_tether_net(**{**LINKS, "stiffness": 0.008 * 500.0 * 3600.0, "damping": 0.0})
    s.set_tether_net(**{**LINKS, "links": LINKS["links"][:3], "length": 5.0, "stiffness": 0.008 * 500.0 * 3600.0, "damping": 0.0})   # two lines carry it
    s.clear_tether_net()
    with pytest.raises(ValueError, match="fp32 range"):
        s.set_tether_net(**{**LINKS, "fairlead_b": (1e39, 0.0, 0.0), "stiffness": 0.0})
    assert s.tether_net is None and s.engine.calls == []


# ---- the helper ------------------------------------------------------------------------------------------------------------------
def test_tether_net_layers_greedily_in_the_callers_order_and_refuses_bad_values():
    links = [[1, 2], [2, 3], [3, 1], [70, 65], [1, 2], [5, 6]]
    t = TetherNet(links, fairlead_a=(0.1, 0.0, -0.5), fairlead_b=(0.0, 0.0, 1.0), length=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], stiffness=7200.0, damping=600.0, n=130)
    # each link the lowest layer free at both of its bodies: a triangle needs three, the bridle (1, 2) twice the fourth
    assert t.layer.tolist() == [0, 1, 2, 0, 3, 0] and t.layers == 4 and t.n == 130 and t.record.shape == (130, 28) and t.record.dtype == np.float64
    again = TetherNet(links, fairlead_a=(0.1, 0.0, -0.5), fairlead_b=(0.0, 0.0, 1.0), length=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], stiffness=7200.0, damping=600.0, n=130)
    assert np.array_equal(again.record, t.record) and np.array_equal(again.layer, t.layer)         # deterministic
    for l, rec in enumerate(tnr.layers_of(t.record)):              # every layer is a Tether's record
        w = t.layer == l
        want = Tether(np.array(links)[w], (0.1, 0.0, -0.5), (0.0, 0.0, 1.0), length=np.arange(1.0, 7.0)[w], stiffness=7200.0, damping=600.0, n=130)
        assert np.array_equal(rec, want.record)
    assert t.record[1, 0:7].tolist() == [0.1, 0.0, -0.5, 1.0, 7200.0, 600.0, 2.0] and t.record[1, 14:21].tolist() == [0.0, 0.0, 1.0, 3.0, 7200.0, 600.0, 3.0]
    assert t.record[2, 21:28].tolist() == [0.0, 0.0, 1.0, 5.0, 7200.0, 600.0, 1.0] and t.record[0].tolist() == [0, 0, 0, 0, 0, 0, 0] * 4
    # another order, other layers
    assert TetherNet(links[::-1], length=1.0, stiffness=1.0, n=130).layer.tolist() == [0, 0, 0, 1, 2, 3]
    # layers as given, taken as they stand; a clash is Tether's refusal
    given = TetherNet(links, length=1.0, stiffness=1.0, n=130, layer=[3, 0, 1, 2, 2, 3])
    assert given.layer.tolist() == [3, 0, 1, 2, 2, 3] and given.layers == 4
    with pytest.raises(ValueError, match="body 2 is in two pairs"):
        TetherNet(links, length=1.0, stiffness=1.0, n=130, layer=[0, 0, 1, 2, 2, 3])
    with pytest.raises(ValueError, match=r"layer is outside 0 \.\. 3"):
        TetherNet(links, length=1.0, stiffness=1.0, n=130, layer=[0, 1, 2, 0, 4, 0])
    with pytest.raises(ValueError, match=r"layer must be \(6,\) integers"):
        TetherNet(links, length=1.0, stiffness=1.0, n=130, layer=[0, 1, 2])
    # nobody tethered and one link as (2,) are legal: one layer
    assert TetherNet(np.zeros((0, 2), int), length=1.0, stiffness=1.0, n=3).record.shape == (3, 7)
    assert TetherNet([0, 1], length=0.0, stiffness=0.0, n=2).layers == 1
    good = dict(links=[[0, 1], [1, 2]], length=5.0, stiffness=7200.0, damping=600.0, n=200)
    nan, inf = float("nan"), float("inf")
    for key in ("length", "stiffness", "damping"):
        for bad in (nan, inf, -inf):
            with pytest.raises(ValueError, match="non-finite"):
                TetherNet(**{**good, key: bad})
        with pytest.raises(ValueError, match=">= 0"):
            TetherNet(**{**good, key: -1e-9})
    for key in ("fairlead_a", "fairlead_b"):
        with pytest.raises(ValueError, match="non-finite"):
            TetherNet(**{**good, key: (0.0, nan, 0.0)})
        with pytest.raises(ValueError, match=r"\(3,\) or \(m, 3\)"):
            TetherNet(**{**good, key: (0.0, 1.0)})
    with pytest.raises(ValueError, match="does not fit 2 links"):
        TetherNet(**{**good, "length": [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError, match="body 5 is tied to itself"):
        TetherNet(**{**good, "links": [[0, 1], [5, 5]]})
    with pytest.raises(ValueError, match="outside 0 .. 199"):
        TetherNet(**{**good, "links": [[0, 200]]})
    with pytest.raises(ValueError, match="outside 0 .. 199"):
        TetherNet(**{**good, "links": [[-1, 3]]})
    with pytest.raises(ValueError, match=r"bodies 63 and 64 lie in tiles 0 and 1; a pair must lie inside one block of 64 bodies.*lay the pair out inside one block of 64"):
        TetherNet(**{**good, "links": [[62, 63], [63, 64]]})
    with pytest.raises(ValueError, match=r"\(m, 2\) integer"):
        TetherNet(**{**good, "links": [[0.0, 1.0]]})
    # a fifth line at a body finds no layer: the link and the body are named
    star = [[9, b] for b in (1, 2, 3, 4)]
    assert TetherNet(star, length=1.0, stiffness=1.0, n=64).layers == 4
    with pytest.raises(ValueError, match=r"link 4 \(9, 5\) finds no free layer: body 9 already has 4 lines"):
        TetherNet(star + [[9, 5]], length=1.0, stiffness=1.0, n=64)
    with pytest.raises(ValueError, match=r"link 4 \(5, 9\) finds no free layer: body 9 already has 4 lines"):
        TetherNet(star + [[5, 9]], length=1.0, stiffness=1.0, n=64)


def test_a_chain_costs_two_layers_and_never_three():
    for bodies in ([0, 1, 2, 3, 4], [10, 3, 40, 7, 63, 0, 31, 32], list(range(64))):
        c = TetherNet.chain(bodies, fairlead_up=(0.0, 0.0, 0.5), fairlead_down=(0.0, 0.0, -0.5), length=1.0, stiffness=10.0, damping=1.0, n=64)
        m = len(bodies) - 1
        assert c.layers == 2 and c.layer.tolist() == [i % 2 for i in range(m)] and c.links.tolist() == [[bodies[i], bodies[i + 1]] for i in range(m)]
        assert c.record.shape == (64, 14)
        # a link leaves the upper body at its lower fairlead and reaches the lower body at its upper one
        b1 = bodies[1]
        assert c.record[bodies[0], 0:3].tolist() == [0.0, 0.0, -0.5] and c.record[b1, 0:3].tolist() == [0.0, 0.0, 0.5] and c.record[b1, 7:10].tolist() == [0.0, 0.0, -0.5]
    assert TetherNet.chain([0, 1, 2, 3, 4], length=1.0, stiffness=1.0, n=5).layer.tolist() == [0, 1, 0, 1]           # layer 0: (0,1) (2,3); layer 1: (1,2) (3,4)
    # the greedy order of an unlucky caller would take three: the chain's explicit layers are the point
    assert TetherNet([[1, 2], [3, 4], [2, 3], [0, 1]], length=1.0, stiffness=1.0, n=5).layers == 2
    assert TetherNet([[0, 1], [2, 3], [4, 5], [1, 2], [3, 4], [5, 0]], length=1.0, stiffness=1.0, n=6).layers == 2
    assert TetherNet([[0, 1], [2, 3], [1, 2], [3, 0], [0, 2]], length=1.0, stiffness=1.0, n=6).layers == 3
    for bad in ([3], [], [[0, 1]]):
        with pytest.raises(ValueError, match="at least two body indices"):
            TetherNet.chain(bad, length=1.0, stiffness=1.0, n=5)


def test_for_chain_and_the_per_body_rule():
    for dt in (1 / 60, 1 / 120):
        for masses in ([500.0, 25.0, 25.0, 25.0, 25.0], [2.0, 500.0], [7.0, 7.0, 7.0]):
            k, c = TetherNet.for_chain(masses, dt)
            m = np.array(masses)
            degree = np.where((np.arange(len(m)) == 0) | (np.arange(len(m)) == len(m) - 1), 1, 2)
            assert (2 * degree * k * dt * dt / m).max() == pytest.approx(DEFAULT_K, rel=1e-13)
            assert (2 * degree * c * dt / m).max() == pytest.approx(DEFAULT_C, rel=1e-13)
            chain = lambda k, c: TetherNet.chain(np.arange(len(m)), length=1.0, stiffness=k, damping=c, n=len(m))  # noqa: E731
            chain(k, c).check_stable(masses, dt)
            chain(k * STABLE / DEFAULT_K, c * STABLE / DEFAULT_C).check_stable(masses, dt)          # the bound itself
            with pytest.raises(ValueError, match=r"2 sum\(k\) dt\^2 / m = 0.0404"):
                chain(1.01 * k * STABLE / DEFAULT_K, c).check_stable(masses, dt)
            with pytest.raises(ValueError, match=r"2 sum\(c\) dt / m = 0.0404"):
                chain(k, 1.01 * c * STABLE / DEFAULT_C).check_stable(masses, dt)
    # stricter than Tether.for_pair for a lone pair: equal masses the same bound, unequal ones m_min / 2 against mu
    dt = 1 / 60
    assert TetherNet.for_chain([500.0, 500.0], dt)[0] == pytest.approx(Tether.for_pair(500.0, 500.0, dt)[0], rel=1e-13)
    assert TetherNet.for_chain([2.0, 500.0], dt)[0] < Tether.for_pair(2.0, 500.0, dt)[0]
    # links that are each stable as a PAIR, an interior body that breaks the per-body rule: 0 - 1 - 2 of 500, 25 and 500 kg,
    # mu = 23.8 kg per link; k at 0.9 of the pair bound gives the middle body 2 * 2 k dt^2 / 25 = 0.137
    masses = [500.0, 25.0, 500.0]
    mu = 500.0 * 25.0 / 525.0
    k = 0.9 * STABLE * mu / dt ** 2
    for pair in ([[0, 1]], [[1, 2]]):
        Tether(pair, length=1.0, stiffness=k, n=3).check_stable(masses, dt)
    with pytest.raises(ValueError, match=r"body 1 \(2 lines\) has 2 sum\(k\) dt\^2 / m = 0.137"):
        TetherNet.chain([0, 1, 2], length=1.0, stiffness=k, n=3).check_stable(masses, dt)
    for bad in (dict(masses=[1.0, 0.0], dt=dt), dict(masses=[1.0, -1.0], dt=dt), dict(masses=[500.0, 1.0], dt=0.0), dict(masses=[5.0], dt=dt)):
        with pytest.raises(ValueError):
            TetherNet.for_chain(**bad)


# ---- the host restatement ------------------------------------------------------------------------------------------------------------
def _random_net(n, seed):
    """n bodies (a multiple of 64) in random poses, every tile one closed chain 0 - 1 - ... - 63 - 0 plus chords i <-> i + 32 on every
    other body: three lines at half the bodies; a third of the links each taut, slack, without stiffness."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 13))
    st[:, 0:3] = rng.uniform(-20, 20, (n, 3))
    q = rng.normal(size=(n, 4))
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))
    st[:, 7:13] = rng.uniform(-1, 1, (n, 6))
    i = np.arange(n)
    ring = np.stack([i, (i // 64) * 64 + (i + 1) % 64], axis=1)
    chords = np.stack([i[(i % 64 < 32) & (i % 2 == 0)], i[(i % 64 < 32) & (i % 2 == 0)] + 32], axis=1)
    links = np.concatenate([ring, chords])
    rng.shuffle(links)
    m = len(links)
    fa, fb = rng.uniform(-0.6, 0.6, (m, 3)), rng.uniform(-0.6, 0.6, (m, 3))
    P = lambda b, f: st[b, 0:3] + np.einsum("nab,nb->na", tr.rot(st[b, 3:7]), f)  # noqa: E731
    l = np.linalg.norm(P(links[:, 1], fb) - P(links[:, 0], fa), axis=1)
    kind = np.arange(m) % 3
    L0 = np.where(kind == 0, l * rng.uniform(0.9, 0.999, m), l * rng.uniform(1.001, 1.2, m))
    k = np.where(kind == 2, 0.0, rng.uniform(100, 8000, m))
    c = np.where(kind == 2, 0.0, rng.uniform(0, 600, m))
    return st, TetherNet(links, fa, fb, length=L0, stiffness=k, damping=c, n=n), kind


def test_host_restatement_is_the_sum_of_the_layers_and_tensions_come_in_the_callers_order():
    st, net, kind = _random_net(192, 41)
    assert net.layers in (3, 4) and (net.layer >= 2).sum() > 10
    recs = tnr.layers_of(net.record)
    ref = sum(tr.wrench(r, st) for r in recs)
    got = net.wrench(st)
    assert np.abs(ref).max() > 1000.0 and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(got - tnr.wrench(net.record, st)).max() <= 1e-12 * np.abs(ref).max()
    # per link, in the caller's order: the reference's tension of the link's layer at either of its bodies
    T = net.tensions(st)
    assert T.shape == (len(net.links),)
    want = np.array([tr.tension(recs[l], st)[a] for (a, b), l in zip(net.links, net.layer)])
    other = np.array([tr.tension(recs[l], st)[b] for (a, b), l in zip(net.links, net.layer)])
    assert np.array_equal(want, other) and np.abs(T - want).max() <= 1e-12 * want.max()
    assert (T[kind == 0] > 0).mean() > 0.8 and not T[kind != 0].any()
    # the forces of a net cancel over each tile: every line pulls its two bodies with opposite forces
    assert np.abs(got[:, 0:3].reshape(3, 64, 3).sum(axis=1)).max() <= 1e-9 * np.abs(ref).max()


def test_the_designed_net_is_what_it_was_designed_to_be():
    st, _, _, net, groups = net_population()
    check_net(st, net, groups)


# ---- the physics -------------------------------------------------------------------------------------------------------------------------
def test_a_free_chain_keeps_its_momentum_to_the_rounding_of_the_additions():
    """No water, no gravity: the lines are the only forces, F on one body and -F on the other per line.  In exact arithmetic the
    total momentum would not move.  The step rounds each body's summed wrench to fp32 once - half an ulp of F_i at most, which
    moves the momentum by dt ulp(F_i) / 2 (a body with ONE line gets that line's force exactly rounded, and its partner the same
    number negated; a body between two lines gets the rounded sum) - and each new velocity v + dt F / m to fp32 once, m ulp(v') / 2.
    Per step the total momentum moves by at most sum_bodies (m ulp(v') + dt ulp(F)) / 2 per axis - the bound formed here step
    by step - plus fp64 dust."""
    dt = float(np.float32(1.0 / 60.0))
    n = 4
    st, pv, pr = np.zeros((n, 13), np.float32), np.zeros((n, 6), np.float32), np.zeros((n, 11), np.float32)
    pr[:, 0:3], pr[:, 10] = (0.4, 0.5, 0.6), (2.0, 5.0, 3.0, 9.0)
    st[:, 6] = 1.0
    st[:, 0:3] = [(0.0, 0.0, 0.0), (1.5, 0.2, -0.1), (3.0, -0.1, 0.3), (4.4, 0.3, 0.1)]
    st[:, 7:10] = [(-0.6, 0.1, 0.0), (-0.1, -0.05, 0.1), (0.2, 0.1, -0.1), (0.7, -0.05, 0.2)]
    st[1, 10:13], st[2, 10:13] = (0.3, -0.2, 0.5), (-0.4, 0.1, 0.2)
    k, c = TetherNet.for_chain(pr[:, 10], dt)
    chain = TetherNet.chain(np.arange(n), fairlead_up=(-0.15, 0.0, 0.0), fairlead_down=(0.15, 0.0, 0.05), length=1.0, stiffness=k, damping=c, n=n)
    chain.check_stable(pr[:, 10], dt)
    run = tnr.closed_loop_net(st, pv, pr, 1025.0, 0.0, dt, 240, net=chain.record, implicit=False, hydro=False)
    m = pr[:, 10].astype(np.float64)
    p0 = (m[:, None] * st[:, 7:10].astype(np.float64)).sum(axis=0)
    bound, p_before = np.zeros(3), p0
    pulled, both = 0, 0
    for r in run:
        F = r["wrench"][:, 0:3]
        assert np.abs(r["net_line"][:, 0:3].sum(axis=0)).max() <= 1e-12                             # equal and opposite per line, in fp64
        T = r["net_tension"]
        pulled += bool(F.any())
        both += bool(T[0, 1] > 0 and T[1, 1] > 0)
        v = r["state"][:, 7:10]
        step_bound = (0.5 * m[:, None] * np.spacing(np.abs(v)).astype(np.float64) + 0.5 * dt * np.spacing(np.abs(F)).astype(np.float64)).sum(axis=0) + 1e-13
        p = (m[:, None] * v.astype(np.float64)).sum(axis=0)
        assert (np.abs(p - p_before) <= step_bound).all(), (p - p_before, step_bound)      # this step's roundings, and nothing else
        bound, p_before = bound + step_bound, p
        drift = np.abs(p - p0)
    dv = np.abs(run[-1]["state"][:, 7:10] - st[:, 7:10]).max()
    print(f"[free chain] lines pulled in {pulled} of 240 steps (body 1 by both of its lines in {both}) and changed a velocity by {dv:.3f} m/s; "
          f"momentum drift {drift.max():.2e} kg m/s within the roundings {bound.max():.2e}")
    assert pulled > 20 and both > 10 and dv > 0.2 and drift.max() < 1e-4


def test_the_hanging_chain_carries_the_submerged_weight_below_each_link():
    """At rest every link carries what hangs below it: 4, 3, 2 and 1 boxes of (25 - 1025 * 0.25^3) * 9.81 = 88.14 N each,
    whatever the stiffness.  Step count and thresholds: the module's docstring."""
    st, pv, pr, sc, dt, hang = hanging_chain()
    k, c = TetherNet.for_chain(pr[:, 10], dt)
    k, c = k * 0.5 * STABLE / DEFAULT_K, c * 0.5 * STABLE / DEFAULT_C                               # half the stability bound
    assert (k, c) == (pytest.approx(450.0, rel=1e-6), pytest.approx(7.5, rel=1e-6))
    assert hanging_constants(pr, dt) == (pytest.approx(k, rel=1e-12), pytest.approx(c, rel=1e-12))
    chain = TetherNet.chain(np.arange(5), length=LINK, stiffness=k, damping=c, n=5)
    chain.check_stable(pr[:, 10], dt)
    run = tnr.closed_loop_net(st, pv, pr, sc.rho, sc.g, dt, HANG_STEPS, net=chain.record, implicit=True)
    s = run[-1]["state"].astype(np.float64)
    speed, T = np.linalg.norm(s[:, 7:10], axis=1), chain.tensions(s)
    print(f"[hanging chain] |v| <= {speed.max():.3e} m/s (threshold {HANG_SPEED:g})  T " + " ".join(f"{t:.2f}" for t in T) + " N  weight below "
          + " ".join(f"{w:.2f}" for w in hang) + f" N  |T - weight| <= {np.abs(T - hang).max():.4f} N (threshold {HANG_TENSION:g})  z "
          + " ".join(f"{z:+.3f}" for z in s[:, 2]))
    assert hang == pytest.approx([352.55, 264.41, 176.27, 88.14], abs=0.01)
    assert speed.max() < HANG_SPEED
    assert np.abs(T - hang).max() < HANG_TENSION
    before = chain.tensions(run[-1]["input"])                                                     # link i lies in layer i % 2, at body i
    assert np.abs(before - [run[-1]["net_tension"][i % 2, i] for i in range(4)]).max() < 1e-9
    assert np.abs(np.diff(s[:, 2]) + LINK + hang / k).max() < 1e-3                                  # each link stretched by T / k
    assert all((r["net_tension"][[0, 1, 0, 1], [0, 1, 2, 3]] > 0).all() for r in run[-600:])
