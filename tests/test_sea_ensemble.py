"""Sea ensembles (hydro_set_sea_ensemble, hydro_sea_ensemble_sample, hydro_step_fused_tiled_multi_ens;
silver2_isaacsim_amd.sea.SeaEnsemble, jonswap_ensemble, pierson_moskowitz_ensemble) as far as a machine without a GPU can see them:
the C boundary, the Python host's marshalling (with the stand-ins of tests/engine_stand_ins.py), ClosedLoopSim's bookkeeping with a
fake engine under its three runners, SeaEnsemble's mapping and reductions by hand, and - on the fp64 closed loop, member by member -
the condition that makes the device tests' identity mean something: any two members move nearly every body differently.

THE FIGURE (fp64 closed loop, tests/sea_ensemble_harness.py's six members at 64 components over tests/test_statistics_gpu.py's 321
bodies, one implicit step from step 5): for every pair of members the state differs in some bit on at least 9 in 10 of the bodies,
and on some body of every tile."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sea_ensemble_harness as seh
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import sea as sea_mod, simulate
from silver2_isaacsim_amd.sea import SeaEnsemble, SeaSpectrum, SeaState, jonswap, jonswap_ensemble, pierson_moskowitz, pierson_moskowitz_ensemble
from designed_populations import bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from engine_stand_ins import FakeLib, FUSED_HEAD, H, KE, make_engine, N, P13, plain, refused, S, SO, STREAM, T, TILES
from populations import DT, G, RHO
from tether_net_population import net_population
from test_statistics import _sim as stat_sim, COMBOS as STAT_COMBOS, StatEngine

ENTRIES = ("hydro_set_sea_ensemble", "hydro_sea_ensemble_sample", "hydro_step_fused_tiled_multi_ens")
ENTRY = ENTRIES[2]
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
W = T((TILES, 4, 64), 0x98000000)
M3 = T((TILES, 27, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)
N2 = T((TILES, 14, 64), 0xC0000000)
PK = T((TILES, 2, 64), 0xC8000000)
ST = T((TILES, 11, 64), 0xD0000000)
LV = T((TILES, 2, 64), 0xD8000000)


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "added to 0.7.1 (no existing entry changed): hydro_set_sea_ensemble, hydro_sea_ensemble_sample, hydro_step_fused_tiled_multi_ens" \
        in text.split("#define HYDRO_VERSION")[0]
    assert int(re.search(r"#define HYDRO_SEA_ENSEMBLE_MAX\s+(\d+)", code).group(1)) == nat.SEA_ENSEMBLE_MAX == sea_mod.ENSEMBLE_MAX == 1024
    assert int(re.search(r"#define HYDRO_SPECTRUM_WAVES_MAX\s+(\d+)", code).group(1)) == nat.SPECTRUM_WAVES_MAX == 64                 # pinned
    # the _stat entry's signature, the spectrum sample's signature
    assert nat.SIGNATURES[ENTRY] == nat.SIGNATURES["hydro_step_fused_tiled_multi_stat"]
    assert nat.SIGNATURES["hydro_sea_ensemble_sample"] == nat.SIGNATURES["hydro_sea_spectrum_sample"]
    assert nat.SIGNATURES["hydro_set_sea_ensemble"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(nat.SeaSpectrum), ctypes.c_int64, ctypes.c_int64])
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_stat") and proto("hydro_sea_ensemble_sample") == proto("hydro_sea_spectrum_sample")
    for phrase in ("Sea ensemble:", "sea(T) = T / tiles_per_sea", "positive multiple of 64", "partly or wholly past n", "count * 3088 B",
                   "AN ENSEMBLE, A SPECTRUM AND A SEA EXCLUDE EACH OTHER", "hydro_set_sea_ensemble(h, NULL, 0, 0)", "EVERY OTHER ENTRY IGNORES IT",
                   "no ensemble set : the launch and its bits are those of hydro_step_fused_tiled_multi_stat", "comes LAST",
                   "capture current-only members", "multiple of 256 bodies", "DESIGN.md section 31",
                   # out of scope, and said so
                   "members with different component counts", "a per-body index table", "open-loop entries", "the plugin",
                   # the symmetry statement: positive since tests/test_symmetry_gpu.py runs the ensemble
                   "SIGN SYMMETRY: exact, member by member"):
        assert phrase in text, phrase
    assert "a sign-symmetry statement" not in text                # no rung disclaims it any more


def test_the_calls_are_plain_c(tmp_path):
    """The three calls through a C99 compiler at its strictest (compiled, not linked: the prototypes are what is checked)."""
    src = tmp_path / "calls.c"
    src.write_text('#include <stddef.h>\n#include "hydro.h"\n'
                   "int calls(hydro_t *h, const hydro_sea_spectrum_t *m, float *f, void *v, int64_t *rows) {\n"
                   "  int rc = hydro_set_sea_ensemble(h, m, HYDRO_SEA_ENSEMBLE_MAX, 256);\n"
                   "  rc += hydro_set_sea_ensemble(h, NULL, 0, 0);\n"
                   "  rc += hydro_sea_ensemble_sample(h, 64, f, 832, 0, 1.0 / 60.0, f, 256, NULL);\n"
                   "  rc += hydro_step_fused_tiled_multi_ens(h, 64, f, 832, f, 832, 1.0 / 60.0, 4, f, 832, f, 832, 0, 0, NULL,\n"
                   "      f, 1, 4, 13, 1, 1, 0, rows, f, 384, HYDRO_FRAME_WORLD, f, 1088, f, 1728, 3, f, 512, f, 896, 2, f, 128,\n"
                   "      v, 704, f, 128, HYDRO_STAT_Z, HYDRO_STAT_TENSION, 0, NULL);\n"
                   "  return rc; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", str(tmp_path / "calls.o"),
                    str(src)], check=True)


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_ens(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                               None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 1728, 3,
                                               None, 512, None, 896, 2, None, 128, None, 704, None, 128, 2, 6, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    one = (nat.SeaSpectrum * 1)()
    assert lib_.hydro_set_sea_ensemble(None, None, 0, 0) == -1 and lib_.hydro_set_sea_ensemble(None, one, 1, 64) == -1
    assert lib_.hydro_sea_ensemble_sample(None, 64, None, 832, 0, 1 / 60, None, 256, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


class EnsembleLib(FakeLib):
    """FakeLib that reads the array of hydro_sea_spectrum_t and its rows while the call runs (the host's arrays live no longer)."""

    def hydro_set_sea_ensemble(self, h, arr, count, bodies_per_sea):
        h = plain(h)
        if arr is None:
            self.calls.append(("hydro_set_sea_ensemble", (h, None, count, bodies_per_sea)))
            return 0
        got = []
        for m in range(count):
            c = arr[m]
            rows = tuple(tuple(getattr(c.wave[j], f) for f, _ in nat.SeaWave._fields_) for j in range(c.waves))
            got.append((tuple(c.current), c.waves, rows if c.waves else bool(c.wave)))
        self.calls.append(("hydro_set_sea_ensemble", (h, tuple(got), count, bodies_per_sea)))
        return 0


@pytest.fixture
def lib(monkeypatch):
    fake = EnsembleLib()
    monkeypatch.setattr(nat, "_lib", fake)
    return fake


@pytest.fixture
def eng(lib):
    return make_engine(lib)


def test_set_sea_ensemble_marshals_the_array(lib, eng):
    ens = seh.ensemble(11, 200, 1)
    assert ens.count == 4 and eng.ensemble_count is None
    eng.set_sea_ensemble(ens)
    want = tuple((m.current, 11, tuple(m.waves)) for m in ens.members)
    assert lib.calls == [("hydro_set_sea_ensemble", (H, want, 4, 64))] and eng.ensemble_count == 4
    lib.calls.clear()
    cur = SeaEnsemble([SeaSpectrum((0.1, 0.0, 0.0)), SeaSpectrum((0.0, 0.2, 0.0))], 256)     # current-only members: waves 0 and NULL rows
    eng.set_sea_ensemble(cur)
    assert lib.calls == [("hydro_set_sea_ensemble", (H, (((0.1, 0.0, 0.0), 0, False), ((0.0, 0.2, 0.0), 0, False)), 2, 256))] and eng.ensemble_count == 2
    lib.calls.clear()
    eng.set_sea_ensemble(None)
    assert lib.calls == [("hydro_set_sea_ensemble", (H, None, 0, 0))] and eng.ensemble_count is None and eng.spectrum_waves is None and eng.sea_waves is None


def test_sea_ensemble_sample(lib, eng):
    assert eng.sea_ensemble_sample(S, N, 10 ** 6, 0.01, out=W, stream=STREAM) is W
    assert lib.calls == [("hydro_sea_ensemble_sample", (H, 1000, 0x10000000, 832, 10 ** 6, 0.01, 0x98000000, 256, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 4, 64) tensor on cuda:0", eng.sea_ensemble_sample, S, N, 0, 0.01, out=A, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.sea_ensemble_sample, A, N, 0, 0.01, out=W, stream=STREAM)


def test_step_fused_tiled_multi_ens_is_the_stat_call_argument_for_argument(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    cases = [(dict(), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + (None, 0, 1)
              + (None, 0) + (None, 0, 1) + (None, 0) + (None, 0, None, 0, 2, 6) + (0, STREAM)),
             (dict(statistics=ST, levels=LV, channel_a=5, channel_b=0, mooring=M3, mooring_layers=3, tether=N2, layers=2, peaks=PK, extremes=E, control=C,
                   applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + (0xA0000000, 1728, 3)
              + (0xA8000000, 512) + (0xC0000000, 896, 2) + (0xC8000000, 128) + (0xD0000000, 704, 0xD8000000, 128, 5, 0) + (123456789012, STREAM)),
             (dict(statistics=ST, levels=LV, extremes=E, applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0, 1) + (0xA8000000, 512)
              + (None, 0, 1) + (None, 0) + (0xD0000000, 704, 0xD8000000, 128, 2, 6) + (5, STREAM))]
    for kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_ens(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, want)]
        lib.calls.clear()
        eng.step_fused_tiled_multi_stat(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw)
        assert lib.calls == [("hydro_step_fused_tiled_multi_stat", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_ens, S, P13, N, 0.01, 3, 0, frame="local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 11, 64) tensor on cuda:0", eng.step_fused_tiled_multi_ens, S, P13, N, 0.01, 3, 0, E, LV, stream=STREAM)
    refused(lib, "mooring_layers must be in 1 .. 4", eng.step_fused_tiled_multi_ens, S, P13, N, 0.01, 3, 0, ST, LV, 2, 6, M3, 5, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class EnsEngine(StatEngine):
    """tests/test_statistics.py's recording engine with the two calls of the ensemble."""

    def set_sea_ensemble(self, ensemble):
        self.calls.append(("set_sea_ensemble", ensemble))

    def step_fused_tiled_multi_ens(self, cur, old, n, dt, steps, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                   peaks, extremes, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("ens", cur, steps, step0=step0, statistics=statistics, levels=levels, channels=(channel_a, channel_b), mooring=mooring,
                          mooring_layers=mooring_layers, tether=tether, layers=layers, peaks=peaks, extremes=extremes, control=control, applied=applied,
                          frame=frame, log=log)


ENS = SeaEnsemble([SeaSpectrum((0.1, 0.0, 0.0)).add_wave(0.2, 0.06, 0.02, 0.8, 0.3), SeaSpectrum((0.0, 0.3, 0.0)).add_wave(0.1, 0.05, -0.03, 0.9, 1.3)], 64)
# test_statistics.py's combinations without its own spectrum (the slot holds the ensemble), each with and without the statistics
COMBOS = {k: v[:9] for k, v in STAT_COMBOS.items() if not v[9]}


def _sim(monkeypatch, *flags):
    s = stat_sim(monkeypatch, *flags)
    s.engine = EnsEngine()
    return s


@pytest.mark.parametrize("statistics", [False, True], ids=["", "stat"])
@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(COMBOS), ids=list(COMBOS))
def test_the_ens_entry_is_picked_first_with_every_runner_and_cleared_again(monkeypatch, combo, run, statistics):
    recorder, applied, control, bed, spread, line, extremes, net, peaks = COMBOS[combo]
    s = _sim(monkeypatch, *COMBOS[combo])
    view = s.track_statistics() if statistics else None
    s.engine.calls.clear()
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert "ens" not in before and len(before) == 3 and (before == ["stat"] * 3) == statistics
    s.engine.calls.clear()
    s.steps_done = 0
    s._graph = "a captured graph of another entry"
    s.set_sea(ENS)
    assert s.sea is ENS and s.engine.calls == [("set_sea_ensemble", ENS)] and s._graph is None          # no sea was set: nothing to clear first
    s.engine.calls.clear()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "ens" and call["steps"] == k and call["step0"] == done
        if statistics:
            assert call["statistics"] is view.buffer and call["levels"] is view.levels_buffer and call["channels"] == (2, 6)
        else:
            assert call["statistics"] is None and call["levels"] is None and call["channels"] == (nat.STAT_Z, nat.STAT_TENSION)
        assert call["mooring"] is (s.mooring_spread if spread else s.mooring) and call["mooring_layers"] == (3 if spread else 1)
        assert (call["mooring"] is not None) == (spread or line)
        assert call["extremes"] is (s.extremes.buffer if extremes else None)
        assert call["tether"] is s.tether_net and (s.tether_net is not None) == net and call["layers"] == (s.tether_layers if net else 1)
        assert call["peaks"] is (s.link_tensions.buffer if peaks else None)
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the ensemble was set)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_sea()
    assert s.sea is None and s.engine.calls == [("set_sea_ensemble", None)]
    s.engine.calls.clear()
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.engine.calls.clear()
    s.clear_sea()                                                  # a second clear is nothing
    assert s.engine.calls == []


def test_a_sea_a_spectrum_and_an_ensemble_swap_in_the_one_slot(monkeypatch):
    s = _sim(monkeypatch)
    sea, spec = SeaState((0.3, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4), SeaSpectrum((0.2, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4)
    other = SeaEnsemble([SeaSpectrum((0.2, 0.0, 0.0))], 128)
    kinds = {"sea": (sea, "set_sea", "sea"), "spectrum": (spec, "set_sea_spectrum", "irr"), "ensemble": (ENS, "set_sea_ensemble", "ens")}
    done = 0
    for first in kinds:                                            # every direction: each kind after each other kind
        for second in kinds:
            if first == second:
                continue
            (a, set_a, _), (b, set_b, entry_b) = kinds[first], kinds[second]
            s.clear_sea()
            s.set_sea(a)
            s.engine.calls.clear()
            s._graph = "a captured graph of the first kind's entry"
            s.set_sea(b)                                           # the library holds one kind at a time: the other kind goes first
            assert s.engine.calls == [(set_a, None), (set_b, b)] and s.sea is b and s._graph is None, (first, second)
            s.run_resident(2)
            assert s.engine.calls[-1]["method"] == entry_b and s.engine.calls[-1]["step0"] == done
            done += 2
    s.clear_sea()
    s.set_sea(ENS)
    s.engine.calls.clear()
    s.set_sea(other)                                               # ensemble to ensemble: one call
    assert s.engine.calls == [("set_sea_ensemble", other)] and s.sea is other
    # an ensemble that does not cover the sim's 70 bodies is refused before anything is changed
    s.engine.calls.clear()
    with pytest.raises(ValueError, match="do not cover"):
        s.set_sea(SeaEnsemble([SeaSpectrum()], 64))
    assert s.engine.calls == [] and s.sea is other
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_sea(ENS)
    assert s.sea is other and s.engine.calls == []


def test_graph_replays_refuse_members_with_components_and_take_currents(monkeypatch):
    s = _sim(monkeypatch)
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s.set_sea(ENS)
    with pytest.raises(ValueError, match="cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [] and s.steps_done == 0
    s.run(3, graph_steps=32)                                     # fewer steps than a replay: eager, legal
    assert s.steps_done == 3 and [c["method"] for c in s.engine.calls[1:]] == ["ens"] * 3
    s.set_sea(SeaEnsemble([SeaSpectrum((0.3, 0.0, 0.0)), SeaSpectrum((0.0, 0.3, 0.0))], 64))       # current-only members: replays
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]


# ---- SeaEnsemble -----------------------------------------------------------------------------------------------------------------
def test_sea_ensemble_by_hand():
    a, b, c = (SeaSpectrum((0.1 * m, 0.0, 0.0)).add_wave(0.1 + 0.1 * m, 0.3, 0.1 * m, 1.5, 0.2 * m) for m in range(3))
    ens = SeaEnsemble([a, b, c], 128)
    assert ens.members == [a, b, c] and ens.count == 3 and ens.bodies_per_sea == 128 and not isinstance(ens, SeaSpectrum)
    assert [int(ens.sea_of(i)) for i in (0, 127, 128, 255, 256, 383)] == [0, 0, 1, 1, 2, 2]
    assert np.array_equal(ens.sea_of(np.array([5, 130, 300])), [0, 1, 2])
    v = np.arange(384.0)
    sp = ens.split(v)
    assert sp.shape == (3, 128) and sp[1, 0] == 128.0 and sp[2, 127] == 383.0 and np.shares_memory(sp, v)
    assert ens.split(np.zeros((384, 6))).shape == (3, 128, 6)
    part = ens.split(np.arange(300.0))                           # the last member's block is partial: the missing bodies are NaN
    assert part.shape == (3, 128) and part[2, 43] == 299.0 and np.isnan(part[2, 44:]).all() and not np.isnan(part[:2]).any()
    with pytest.raises(ValueError):
        ens.split(np.zeros(385))
    with pytest.raises(ValueError):
        ens.split(np.zeros(300, np.int32))
    # the two reductions, by hand: design d has the maxima (d, 128 + d, 256 + d) over the three members
    mean, std = ens.mean_of_maxima(v), ens.std_of_maxima(v)
    assert mean.shape == std.shape == (128,) and np.array_equal(mean, 128.0 + np.arange(128.0)) and np.allclose(std, 128.0, rtol=1e-15)
    x = np.array([1.0, 2.0, 6.0])
    three = SeaEnsemble([a, b, c], 64)
    vals = np.repeat(x, 64)
    assert np.allclose(three.mean_of_maxima(vals), 3.0) and np.allclose(three.std_of_maxima(vals), np.sqrt(7.0), rtol=1e-15)      # ((2^2 + 1 + 3^2) / 2)^(1/2)
    assert not SeaEnsemble([a], 64).std_of_maxima(np.ones(64)).any()
    # elevation: the member's
    xs, ys, body = np.array([1.0, -2.0, 3.0, 4.0]), np.array([0.5, 0.0, -1.0, 2.0]), np.array([0, 130, 383, 128])
    eta = ens.elevation(xs, ys, 3.7, body)
    for i, m in enumerate((a, b, c, b)):
        assert eta[i] == m.elevation(xs[i], ys[i], 3.7)
    assert len(ens.waves) == 3 and not SeaEnsemble([SeaSpectrum((0.1, 0, 0))], 64).waves
    # refusals
    with pytest.raises(ValueError, match="same number of wave components"):
        SeaEnsemble([a, SeaSpectrum((0.0, 0.0, 0.0))], 64)
    for bad in (0, 63, 96, -64, 64.5):
        with pytest.raises(ValueError, match="multiple of 64"):
            SeaEnsemble([a], bad)
    with pytest.raises(ValueError):
        SeaEnsemble([], 64)
    with pytest.raises(ValueError):
        SeaEnsemble([SeaState()], 64)
    with pytest.raises(ValueError):
        SeaEnsemble([SeaSpectrum()] * 1025, 64)


def test_ensemble_constructors_give_exactly_the_seeded_seas():
    ens = jonswap_ensemble(1.5, 7.0, 25.0, bodies_per_sea=4096, spread="cos2", current=(0.4, 0.0, 0.0))
    assert ens.count == 16 and ens.bodies_per_sea == 4096
    for i, m in enumerate(ens.members):
        want = jonswap(1.5, 7.0, 25.0, seed=i, spread="cos2", current=(0.4, 0.0, 0.0))
        assert m.waves == want.waves and m.current == want.current and isinstance(m, SeaSpectrum)
    heads, curs = [0.0, 90.0, 180.0], [(0.1, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 0.0)]
    pm = pierson_moskowitz_ensemble(2.0, 8.0, heads, seeds=(7, 7, 9), bodies_per_sea=64, current=curs, components=11)
    for m, hd, cu, sd in zip(pm.members, heads, curs, (7, 7, 9)):
        want = pierson_moskowitz(2.0, 8.0, hd, seed=sd, current=cu, components=11)
        assert m.waves == want.waves and m.current == want.current and len(m.waves) == 11
    js = jonswap_ensemble(1.0, 6.0, 10.0, seeds=range(3), bodies_per_sea=128, gamma=2.0)
    assert [m.waves for m in js.members] == [jonswap(1.0, 6.0, 10.0, seed=s, gamma=2.0).waves for s in range(3)]
    with pytest.raises(ValueError, match="one per member"):
        jonswap_ensemble(1.0, 6.0, [0.0, 10.0], seeds=range(3), bodies_per_sea=64)
    with pytest.raises(ValueError, match="one per member"):
        jonswap_ensemble(1.0, 6.0, 0.0, seeds=range(3), bodies_per_sea=64, current=[(0.0, 0.0, 0.0)] * 2)


# ---- the condition that makes the identity mean something ------------------------------------------------------------------------------
def test_the_members_move_nearly_every_body_differently_on_the_fp64_closed_loop(bed_pop):
    """One implicit step of the fp64 closed loop from step 5 under each of the six members (64 components) over the device tests' 321
    bodies: for every pair of members the states differ on >= 9 in 10 of the bodies and in every tile - so "member 0 for everyone" or
    "the neighbour's table" cannot pass the device tests' identity on any tile.  Eleven components likewise."""
    _, _, params, _, _ = bed_pop
    st, pv, _, _, _ = net_population()
    st, pv = st[:321], pv[:321]
    for waves in (64, 11):
        states = [closed_loop(st, pv, params["f32"][:321], RHO, G, DT, 1, sea=m, step0=5, implicit=True)[0]["state"] for m in seh.members(waves)]
        fraction, every_tile = seh.apart(states, 321)
        print(f"[members apart, {waves} components] the closest pair differs on {fraction:.1%} of 321 bodies; in every tile: {every_tile}")
        assert fraction >= 0.9 and every_tile
        for n in (65, 200):
            f, t = seh.apart(states, n)
            assert f >= 0.9 and t, n


# ---- the recorded figures ---------------------------------------------------------------------------------------------------------
def test_recorded_isa_figures_meet_the_conditions_of_the_rung():
    """profiles/sea_ensemble.json (scripts/diag_sea_ensemble.py --isa-only): each of the 2 x 32 instantiations stays within 168 VGPRs at
    three waves per SIMD, uses no scratch, has byte for byte the LDS of the kernel it is built on, and reads its table with scalar
    loads only in every one of its four component loops."""
    import json
    isa = json.load(open(os.path.join(REPO, "profiles", "sea_ensemble.json")))["isa"]
    per = isa["per_instantiation"]
    assert len(per) == 64 and isa["conditions_met"] is True
    assert sum("ens_stat" in name for name in per) == 32
    for name, row in per.items():
        assert row["scratch_bytes"] == 0 and row["vgprs"] <= 168 and row["waves_per_simd"] >= 3, name
        assert row["lds_bytes"] == row["built_on_lds_bytes"] <= 54613, name
        assert row["component_loops"] == 4 and row["component_loop_scalar_loads"] > 0, name
        assert row["component_loop_lds"] == 0 and row["component_loop_vector_memory"] == 0, name
