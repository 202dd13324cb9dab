"""Finite-depth seas (hydro_set_sea_finite_depth, hydro_sea_finite_depth_sample, hydro_step_fused_tiled_multi_fd;
silver2_isaacsim_amd.sea.wavenumber, the `depth` of SeaSpectrum and SeaEnsemble) as far as a machine without a GPU can see them:
the C boundary, the Python host's marshalling (with the stand-ins of tests/engine_stand_ins.py), ClosedLoopSim's bookkeeping with a
fake engine under its three runners, the dispersion relation, the fp64 velocity profiles, the fp32 emulation of the header's
arithmetic with the bound it fixes for the device (tests/sea_depth_reference.py), and - on the fp64 closed loop - the condition
that makes the device tests mean something: at kappa_p h = 1 the bottom moves nearly every body.

THE FIGURES (printed by the tests): the emulation stands 3.18 units of 2^-24 from fp64 cosh / sinh (eta 2.34, u 3.18), so
DEPTH_VIEW_BOUND = 8; the same reference without the G term misses the emulation by 8e5 units.  On the fp64 closed loop, one
implicit step from step 5 over the sea-ensemble tests' 321 bodies: the state at h = 9 m differs from the deep one on every one of
the bodies, in every tile, for every member and for 11 and 64 components."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sea_depth_reference as sdr
import sea_ensemble_harness as seh
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import sea as sea_mod, simulate
from silver2_isaacsim_amd.sea import (SeaEnsemble, SeaSpectrum, SeaState, jonswap, jonswap_ensemble, pierson_moskowitz, pierson_moskowitz_ensemble,
                                      wavenumber)
from designed_populations import bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from engine_stand_ins import FUSED_HEAD, H, KE, make_engine, N, P13, plain, refused, S, SO, STREAM, T, TILES
from populations import DT, G, RHO
from tether_net_population import net_population
from test_sea_ensemble import COMBOS, EnsEngine, EnsembleLib
from test_statistics import _sim as stat_sim

ENTRIES = ("hydro_set_sea_finite_depth", "hydro_sea_finite_depth_sample", "hydro_step_fused_tiled_multi_fd")
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
    assert "added to 0.7.1 (no existing entry changed): hydro_set_sea_finite_depth, hydro_sea_finite_depth_sample," in text.split("#define HYDRO_VERSION")[0]
    assert nat.SIGNATURES[ENTRY] == nat.SIGNATURES["hydro_step_fused_tiled_multi_ens"]
    assert nat.SIGNATURES["hydro_sea_finite_depth_sample"] == nat.SIGNATURES["hydro_sea_ensemble_sample"]
    assert nat.SIGNATURES["hydro_set_sea_finite_depth"] == (ctypes.c_int, nat.SIGNATURES["hydro_set_sea_ensemble"][1] + [ctypes.c_double])
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_ens") and proto("hydro_sea_finite_depth_sample") == proto("hydro_sea_ensemble_sample")
    assert proto("hydro_set_sea_finite_depth") == proto("hydro_set_sea_ensemble") + ", double depth"
    for phrase in ("Finite-depth sea:", "zc    = max(min(z_rel, 0), -h)", "G_j   = exp2(fma(-kl2_j, zc, gl_j))", "gl_j = -2 kappa_j h log2(e)",
                   "u_x = fma(cx_j, (E_j + G_j) * c_j, u_x)", "u_z = fma(aw_j, (E_j - G_j) * s_j, u_z)", "times 1 / (1 - q_j)",
                   "cosh(kappa (zc + h)) / sinh(kappa h)", "sinh(kappa (zc + h)) / sinh(kappa h)", "ascending j, eta from +0 and u from U",
                   "omega^2 = g kappa tanh(kappa h) is the caller's business", "+-inf and NaN included", "IT IS THE FOURTH KIND OF SEA",
                   "hydro_set_sea_finite_depth(h, NULL, 0, 0, 0)", "EVERY OTHER ENTRY IGNORES A FINITE-DEPTH SEA",
                   "no finite-depth sea set : the launch and its bits are those of hydro_step_fused_tiled_multi_ens", "Set z_b = -h", "DESIGN.md section 32",
                   # out of scope, and said so
                   "depth-limited spectral shape (TMA)", "shoaling, breaking and a sloping bed", "depth in the 8-wave", "open-loop entries", "the plugin",
                   "members of different depths",
                   # the symmetry statement: positive since tests/test_symmetry_gpu.py runs this rung
                   "SIGN SYMMETRY: exact at any depth",
                   # the sentences about the deep entries stay: they remain true of the entries they describe
                   "finite depth", "stays the deep-water one however shallow z_b makes the scene"):
        assert phrase in text, phrase
    assert "a sign-symmetry statement" not in text                # no rung disclaims it any more


def test_the_calls_are_plain_c(tmp_path):
    """The three calls through a C99 compiler at its strictest (compiled, not linked: the prototypes are what is checked)."""
    src = tmp_path / "calls.c"
    src.write_text('#include <stddef.h>\n#include "hydro.h"\n'
                   "int calls(hydro_t *h, const hydro_sea_spectrum_t *m, float *f, void *v, int64_t *rows) {\n"
                   "  int rc = hydro_set_sea_finite_depth(h, m, HYDRO_SEA_ENSEMBLE_MAX, 256, 20.0);\n"
                   "  rc += hydro_set_sea_finite_depth(h, NULL, 0, 0, 0.0);\n"
                   "  rc += hydro_sea_finite_depth_sample(h, 64, f, 832, 0, 1.0 / 60.0, f, 256, NULL);\n"
                   "  rc += hydro_step_fused_tiled_multi_fd(h, 64, f, 832, f, 832, 1.0 / 60.0, 4, f, 832, f, 832, 0, 0, NULL,\n"
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
    rc = lib_.hydro_step_fused_tiled_multi_fd(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                              None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 1728, 3,
                                              None, 512, None, 896, 2, None, 128, None, 704, None, 128, 2, 6, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    one = (nat.SeaSpectrum * 1)()
    assert lib_.hydro_set_sea_finite_depth(None, None, 0, 0, 0.0) == -1 and lib_.hydro_set_sea_finite_depth(None, one, 1, 64, 20.0) == -1
    assert lib_.hydro_sea_finite_depth_sample(None, 64, None, 832, 0, 1 / 60, None, 256, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


class DepthLib(EnsembleLib):
    """tests/test_sea_ensemble.py's stand-in, which reads the array of hydro_sea_spectrum_t while the call runs, with the depth's setter."""

    def hydro_set_sea_finite_depth(self, h, arr, count, bodies_per_sea, depth):
        self.hydro_set_sea_ensemble(h, arr, count, bodies_per_sea)
        name, args = self.calls.pop()
        self.calls.append(("hydro_set_sea_finite_depth", args + (depth,)))
        return 0


@pytest.fixture
def lib(monkeypatch):
    fake = DepthLib()
    monkeypatch.setattr(nat, "_lib", fake)
    return fake


@pytest.fixture
def eng(lib):
    return make_engine(lib)


def test_set_sea_finite_depth_marshals_members_and_depth(lib, eng):
    ens = SeaEnsemble([sdr.with_depth(m, 20.0) for m in seh.members(11, 4)], 64)
    assert ens.depth == 20.0 and eng.finite_depth is None
    eng.set_sea_finite_depth(ens)
    want = tuple((m.current, 11, tuple(m.waves)) for m in ens.members)
    assert lib.calls == [("hydro_set_sea_finite_depth", (H, want, 4, 64, 20.0))] and eng.finite_depth == 20.0 and eng.ensemble_count is None
    lib.calls.clear()
    # a lone spectrum rides as ONE member whose block covers the engine's bodies (1000: 16 tiles), or the n it is told
    spec = sdr.with_depth(seh.members(11)[1], 7.5)
    eng.set_sea_finite_depth(spec)
    assert lib.calls == [("hydro_set_sea_finite_depth", (H, ((spec.current, 11, tuple(spec.waves)),), 1, 1024, 7.5))] and eng.finite_depth == 7.5
    lib.calls.clear()
    eng.set_sea_finite_depth(spec, n=65)
    assert lib.calls[0][1][2:] == (1, 128, 7.5)
    lib.calls.clear()
    eng.set_sea_finite_depth(SeaSpectrum((0.1, 0.0, 0.0), depth=3.0))          # current-only: waves 0 and NULL rows
    assert lib.calls == [("hydro_set_sea_finite_depth", (H, (((0.1, 0.0, 0.0), 0, False),), 1, 1024, 3.0))]
    lib.calls.clear()
    no_depth = "a finite-depth sea needs a depth (SeaSpectrum(depth=), jonswap(..., depth=))"
    refused(lib, no_depth, eng.set_sea_finite_depth, seh.members(11)[0])
    refused(lib, no_depth, eng.set_sea_finite_depth, seh.ensemble(11, 200, 1))
    assert eng.finite_depth == 3.0
    eng.set_sea_finite_depth(None)
    assert lib.calls == [("hydro_set_sea_finite_depth", (H, None, 0, 0, 0.0))] and eng.finite_depth is None and eng.spectrum_waves is None


def test_sea_finite_depth_sample(lib, eng):
    assert eng.sea_finite_depth_sample(S, N, 10 ** 6, 0.01, out=W, stream=STREAM) is W
    assert lib.calls == [("hydro_sea_finite_depth_sample", (H, 1000, 0x10000000, 832, 10 ** 6, 0.01, 0x98000000, 256, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 4, 64) tensor on cuda:0", eng.sea_finite_depth_sample, S, N, 0, 0.01, out=A, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.sea_finite_depth_sample, A, N, 0, 0.01, out=W, stream=STREAM)


def test_step_fused_tiled_multi_fd_is_the_ens_call_argument_for_argument(lib, eng):
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
        assert eng.step_fused_tiled_multi_fd(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, want)]
        lib.calls.clear()
        eng.step_fused_tiled_multi_ens(S, P13, N, 0.01, 7, step0, state_out=state_out, stream=STREAM, **kw)
        assert lib.calls == [("hydro_step_fused_tiled_multi_ens", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_fd, S, P13, N, 0.01, 3, 0, frame="local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 11, 64) tensor on cuda:0", eng.step_fused_tiled_multi_fd, S, P13, N, 0.01, 3, 0, E, LV, stream=STREAM)
    refused(lib, "mooring_layers must be in 1 .. 4", eng.step_fused_tiled_multi_fd, S, P13, N, 0.01, 3, 0, ST, LV, 2, 6, M3, 5, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------
class FdEngine(EnsEngine):
    """tests/test_sea_ensemble.py's recording engine with the two calls of the finite-depth sea."""

    def set_sea_finite_depth(self, sea):
        self.calls.append(("set_sea_finite_depth", sea))

    def step_fused_tiled_multi_fd(self, cur, old, n, dt, steps, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                  peaks, extremes, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("fd", cur, steps, step0=step0, statistics=statistics, levels=levels, channels=(channel_a, channel_b), mooring=mooring,
                          mooring_layers=mooring_layers, tether=tether, layers=layers, peaks=peaks, extremes=extremes, control=control, applied=applied,
                          frame=frame, log=log)


FD_SPEC = SeaSpectrum((0.1, 0.0, 0.0), depth=12.0).add_wave(0.2, 0.06, 0.02, 0.8, 0.3)
FD_ENS = SeaEnsemble([SeaSpectrum((0.1, 0.0, 0.0), 12.0).add_wave(0.2, 0.06, 0.02, 0.8, 0.3), SeaSpectrum((0.0, 0.3, 0.0), 12.0).add_wave(0.1, 0.05, -0.03, 0.9, 1.3)], 64)


def _sim(monkeypatch, *flags):
    s = stat_sim(monkeypatch, *flags)
    s.engine = FdEngine()
    return s


@pytest.mark.parametrize("kind", ["spectrum", "ensemble"])
@pytest.mark.parametrize("statistics", [False, True], ids=["", "stat"])
@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(COMBOS), ids=list(COMBOS))
def test_the_fd_entry_is_picked_first_with_every_runner_and_cleared_again(monkeypatch, combo, run, statistics, kind):
    recorder, applied, control, bed, spread, line, extremes, net, peaks = COMBOS[combo]
    sea = FD_SPEC if kind == "spectrum" else FD_ENS
    s = _sim(monkeypatch, *COMBOS[combo])
    view = s.track_statistics() if statistics else None
    s.engine.calls.clear()
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert "fd" not in before and len(before) == 3
    s.engine.calls.clear()
    s.steps_done = 0
    s._graph = "a captured graph of another entry"
    s.set_sea(sea)
    assert s.sea is sea and s.engine.calls == [("set_sea_finite_depth", sea)] and s._graph is None          # no sea was set: nothing to clear first
    s.engine.calls.clear()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "fd" and call["steps"] == k and call["step0"] == done
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
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the sea was set)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_sea()
    assert s.sea is None and s.engine.calls == [("set_sea_finite_depth", None)]
    s.engine.calls.clear()
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.engine.calls.clear()
    s.clear_sea()                                                  # a second clear is nothing
    assert s.engine.calls == []


def test_the_four_kinds_swap_in_the_one_slot(monkeypatch):
    s = _sim(monkeypatch)
    sea, spec = SeaState((0.3, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4), SeaSpectrum((0.2, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4)
    ens = SeaEnsemble([SeaSpectrum((0.2, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4)], 128)
    kinds = {"sea": (sea, "set_sea", "sea"), "spectrum": (spec, "set_sea_spectrum", "irr"), "ensemble": (ens, "set_sea_ensemble", "ens"),
             "deep spectrum, finite": (FD_SPEC, "set_sea_finite_depth", "fd")}
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
    s.set_sea(FD_SPEC)
    s.engine.calls.clear()
    s.set_sea(FD_ENS)                                              # finite depth to finite depth: one call, spectrum or ensemble
    assert s.engine.calls == [("set_sea_finite_depth", FD_ENS)] and s.sea is FD_ENS
    s.engine.calls.clear()
    with pytest.raises(ValueError, match="do not cover"):          # an ensemble that does not cover the sim's 70 bodies
        s.set_sea(SeaEnsemble([SeaSpectrum(depth=5.0)], 64))
    assert s.engine.calls == [] and s.sea is FD_ENS
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.set_sea(FD_SPEC)
    assert s.sea is FD_ENS and s.engine.calls == []


def test_graph_replays_refuse_components_and_take_currents(monkeypatch):
    s = _sim(monkeypatch)
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    for sea in (FD_SPEC, FD_ENS):
        s.set_sea(sea)
        with pytest.raises(ValueError, match="cannot ride in graph replays"):
            s.run(64, graph_steps=32)
        assert captured == []
    before = s.steps_done
    s.run(3, graph_steps=32)                                     # fewer steps than a replay: eager, legal
    assert s.steps_done == before + 3 and [c["method"] for c in s.engine.calls[-3:]] == ["fd"] * 3
    s.set_sea(SeaSpectrum((0.3, 0.0, 0.0), depth=12.0))          # current-only: replays
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]


# ---- the dispersion relation ------------------------------------------------------------------------------------------------------
def test_wavenumber_solves_the_dispersion_relation():
    g, h = 9.81, 20.0
    x = np.exp(np.linspace(math.log(0.05), math.log(50.0), 400))                     # kappa h
    omega = np.sqrt(g * (x / h) * np.tanh(x))
    kappa = wavenumber(omega, h, g)
    residual = np.abs(g * kappa * np.tanh(kappa * h) - omega ** 2) / omega ** 2
    print(f"[wavenumber] largest relative residual of omega^2 = g kappa tanh(kappa h) over kappa h = 0.05 .. 50: {residual.max():.2e}")
    assert residual.max() <= 1e-12
    assert np.abs(kappa * h - x).max() / 50.0 <= 1e-12 and (np.diff(kappa) > 0.0).all()
    deep = omega[x >= 20.0]
    assert len(deep) and (np.abs(wavenumber(deep, h, g) - deep ** 2 / g) <= 1e-12 * deep ** 2 / g).all()            # tanh(20) = 1 - 3.6e-18
    # shallow water: kappa h tanh(kappa h) = c gives kappa h = sqrt(c) (1 + c / 6 + 11 c^2 / 360 + O(c^3)); the next term is below c^3
    xs = np.exp(np.linspace(math.log(1e-4), math.log(0.05), 60))
    om = np.sqrt(g * (xs / h) * np.tanh(xs))
    c = om ** 2 * h / g
    k = wavenumber(om, h, g)
    assert (np.abs(k / (om / math.sqrt(g * h)) - (1.0 + c / 6.0 + 11.0 * c * c / 360.0)) <= c ** 3 + 1e-12).all()
    assert (np.abs(k / (om / math.sqrt(g * h)) - 1.0) <= c / 6.0 + c * c).all() and (k >= om / math.sqrt(g * h)).all()
    # scalars, zero, and what it refuses
    assert isinstance(wavenumber(0.9, 20.0), float) and wavenumber(0.0, 20.0) == 0.0
    assert wavenumber(0.9, 20.0, 9.81) == pytest.approx(float(wavenumber(np.array([0.9]), 20.0)[0]), rel=0, abs=0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            wavenumber(1.0, bad)
    with pytest.raises(ValueError):
        wavenumber(-1.0, 20.0)


def test_constructors_place_the_same_bins_on_the_depths_wavenumbers():
    for make, kw in ((jonswap, dict(gamma=2.0)), (pierson_moskowitz, {})):
        deep = make(1.5, 7.0, 25.0, components=11, seed=4, spread="cos2", current=(0.4, 0.0, 0.0), **kw)
        fd = make(1.5, 7.0, 25.0, components=11, seed=4, spread="cos2", current=(0.4, 0.0, 0.0), depth=20.0, **kw)
        assert deep.depth is None and fd.depth == 20.0 and fd.current == deep.current and fd.hs() == deep.hs()
        for (a, kx, ky, om, ph), (a2, kx2, ky2, om2, ph2) in zip(deep.waves, fd.waves):
            assert (a, om, ph) == (a2, om2, ph2)                                       # the bins, the amplitudes, the phases
            assert math.atan2(ky, kx) == pytest.approx(math.atan2(ky2, kx2), abs=1e-15)                      # the headings
            assert math.hypot(kx2, ky2) == pytest.approx(wavenumber(om, 20.0), rel=1e-15) and math.hypot(kx2, ky2) > math.hypot(kx, ky)
    ens = jonswap_ensemble(1.5, 7.0, 25.0, seeds=range(3), bodies_per_sea=128, depth=20.0)
    assert ens.depth == 20.0 and [m.waves for m in ens.members] == [jonswap(1.5, 7.0, 25.0, seed=s, depth=20.0).waves for s in range(3)]
    assert pierson_moskowitz_ensemble(1.0, 6.0, 0.0, seeds=range(2), bodies_per_sea=64).depth is None
    assert jonswap_ensemble(1.0, 6.0, 0.0, seeds=range(2), bodies_per_sea=64).depth is None
    with pytest.raises(ValueError, match="same depth"):
        SeaEnsemble([SeaSpectrum(depth=20.0), SeaSpectrum()], 64)
    with pytest.raises(ValueError, match="same depth"):
        SeaEnsemble([SeaSpectrum(depth=20.0), SeaSpectrum(depth=21.0)], 64)
    for bad in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            SeaSpectrum(depth=bad)
    assert sea_mod.SeaSpectrum((0.0, 0.0, 0.0)).depth is None


# ---- the velocity in fp64 -------------------------------------------------------------------------------------------------------
def test_velocity_follows_the_depth_in_fp64():
    h, a, om = 20.0, 0.4, 2.0 * math.pi / 7.0
    kappa = wavenumber(om, h)
    head = math.radians(30.0)
    sea = SeaSpectrum((0.0, 0.0, 0.0), depth=h).add_wave(a, kappa * math.cos(head), kappa * math.sin(head), om, 0.3)
    deep = sdr.with_depth(sea, None)
    x, y, t = np.linspace(-50.0, 50.0, 41), np.linspace(30.0, -30.0, 41), 1.7
    # the surface does not change
    assert np.array_equal(sea.elevation(x, y, t), deep.elevation(x, y, t))
    # u_z = 0 on the bed, whatever the phase
    assert not sea.velocity(x, y, -h, t)[:, 2].any()
    # the horizontal amplitude at z = 0 is a omega coth(kappa h): at the crest (th = 0) and, for u_z, a quarter period on (th = pi / 2)
    crest, quarter = 0.3 / om, (0.3 - 0.5 * math.pi) / om
    u0 = sea.velocity(0.0, 0.0, 0.0, crest)
    assert math.hypot(u0[0], u0[1]) == pytest.approx(a * om / math.tanh(kappa * h), rel=1e-13) and abs(u0[2]) < 1e-15
    assert math.atan2(u0[1], u0[0]) == pytest.approx(head, abs=1e-13)
    assert sea.velocity(0.0, 0.0, 0.0, quarter)[2] == pytest.approx(a * om, rel=1e-13)     # sinh / sinh = 1 at the surface
    ts = np.linspace(0.0, 7.0, 2001)                                                       # (and nowhere in the period is it larger)
    over = sea.velocity(0.0, 0.0, 0.0, ts)
    assert np.hypot(over[:, 0], over[:, 1]).max() <= a * om / math.tanh(kappa * h) * (1.0 + 1e-13)
    # on the bed the motion is horizontal and NOT zero: a omega / sinh(kappa h)
    ub = sea.velocity(0.0, 0.0, -h, crest)
    assert math.hypot(ub[0], ub[1]) == pytest.approx(a * om / math.sinh(kappa * h), rel=1e-13) and ub[2] == 0.0
    # below the bed the water is the bed's; above the surface the surface's
    for z in (-h - 1e-9, -2.0 * h, -1e30, -np.inf):
        assert np.array_equal(sea.velocity(x, y, z, t), sea.velocity(x, y, -h, t))
    assert np.array_equal(sea.velocity(x, y, 3.0, t), sea.velocity(x, y, 0.0, t))
    # against cosh and sinh, at every depth; and the reference module's restatement is the same function
    z = np.linspace(-h, 0.0, 41)
    th = sea.waves[0][1] * x + sea.waves[0][2] * y - om * t + 0.3
    want_h, want_z = a * om * np.cosh(kappa * (z + h)) / math.sinh(kappa * h) * np.cos(th), a * om * np.sinh(kappa * (z + h)) / math.sinh(kappa * h) * np.sin(th)
    got = sea.velocity(x, y, z, t)
    assert np.allclose(np.hypot(got[:, 0], got[:, 1]), np.abs(want_h), rtol=1e-13, atol=1e-16) and np.allclose(got[:, 2], want_z, rtol=1e-13, atol=1e-16)
    eta = sea.elevation(x, y, t)
    _, u = sdr.water(sea, x, y, z + eta, t / DT, DT)
    assert np.allclose(u, got, rtol=1e-12, atol=1e-15)
    # deep water: the deep model's velocity
    far = sdr.with_depth(sea, 1e6)
    assert np.allclose(far.velocity(x, y, z, t), deep.velocity(x, y, z, t), rtol=1e-15, atol=0.0)


# ---- the fp32 emulation and the bound it fixes ------------------------------------------------------------------------------------
def test_the_emulation_fixes_the_bound_and_tells_the_g_term():
    """The header's arithmetic in NumPy fp32 against fp64 cosh / sinh: the largest error over the population (above, at the surface,
    mid-depth, on the bed, below it), steps 0, 1, 7 and 10^6, and 9, 10, 11, 63 and 64 components fixes DEPTH_VIEW_BOUND - the next
    power of two at or above twice it.  The same reference WITHOUT the G term misses by orders of magnitude."""
    full = sdr.designed_sea()
    kp = wavenumber(2.0 * math.pi / sdr.TP, sdr.DEPTH)
    assert 0.9 <= kp * sdr.DEPTH <= 1.1
    st = sdr.population()
    z = st[:, 2].astype(np.float64)
    assert (z > 0.1).any() and (np.abs(z) < 0.8).any() and ((z < -1.0) & (z > -sdr.DEPTH)).any() and (z == -sdr.DEPTH).any() and (z < -sdr.DEPTH).any()
    worst, miss = {"eta": 0.0, "u": 0.0}, np.inf
    for count in (9, 10, 11, 63, 64):
        sea = sdr.truncated(full, count)
        for step in sdr.VIEW_STEPS:
            eta32, u32 = sdr.water_fp32(sea, st[:, 0], st[:, 1], st[:, 2], step, DT)
            for k, v in sdr.view_errors(sea, st, step, DT, eta32, u32).items():
                worst[k] = max(worst[k], v)
            miss = min(miss, sdr.view_errors(sea, st, step, DT, eta32, u32, without_g=True)["u"])
    e = max(worst.values())
    print(f"[depth view, emulated] largest error in units of 2^-24 of the scale: eta {worst['eta']:.2f}  u {worst['u']:.2f}; "
          f"twice that is {2 * e:.2f}: bound {sdr.DEPTH_VIEW_BOUND:g}; without G the reference misses by {miss:.3g}")
    assert sdr.DEPTH_VIEW_BOUND == 2.0 ** math.ceil(math.log2(2.0 * e))
    assert miss > 1000 * sdr.DEPTH_VIEW_BOUND


def test_the_emulation_in_deep_water_is_the_spectrums_bits_and_its_constants_are_the_deep_ones():
    """h = 1e6 m with every kappa_j >= 0.01: q_j == 0.0 in fp64, every G exponent is below -200, and the emulated finite-depth view
    equals tests/sea_spectrum_reference.py's emulation of the deep model bit for bit - the identity the device test asserts."""
    from sea_spectrum_reference import water_fp32 as deep_fp32
    st = sdr.population()
    for sea in seh.members(64):
        consts, q = sdr.device_constants(sea, 1e6)
        assert min(math.hypot(w[1], w[2]) for w in sea.waves) >= 0.01 and all(x == 0.0 for x in q)
        assert all(float(c[7]) + float(c[3]) * 1000.0 < -200.0 for c in consts)
        for step in (0, 7):
            got, want = sdr.water_fp32(sea, st[:, 0], st[:, 1], st[:, 2], step, DT, depth=1e6), deep_fp32(sea, st[:, 0], st[:, 1], st[:, 2], step, DT)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_value_rules_of_the_emulation():
    """p_z = +-inf and NaN leave a finite eta and u: the clamp returns the number."""
    sea = sdr.designed_sea(11)
    st = sdr.population()[:8].copy()
    st[:, 2] = [np.inf, -np.inf, np.nan, 0.0, -sdr.DEPTH, 3e38, -3e38, -1.0]
    eta, u = sdr.water_fp32(sea, st[:, 0], st[:, 1], st[:, 2], 7, DT)
    assert np.isfinite(eta).all() and np.isfinite(u).all()
    surface, bed = sdr.water_fp32(sea, st[:, 0], st[:, 1], np.zeros(8, np.float32) + 50.0, 7, DT)[1], sdr.water_fp32(sea, st[:, 0], st[:, 1], np.full(8, -50.0, np.float32), 7, DT)[1]
    assert np.array_equal(u[[0, 2, 5]], surface[[0, 2, 5]]) and np.array_equal(u[[1, 6]], bed[[1, 6]])


# ---- the condition that makes the device tests mean something ------------------------------------------------------------------------
def test_the_bottom_moves_nearly_every_body_on_the_fp64_closed_loop(bed_pop):
    """One implicit step of the fp64 closed loop from step 5 over the device tests' 321 bodies under each harness member: the state at
    h = 9 m (kappa_p h = 1) differs from the deep one on >= 3 in 4 of the bodies and in every tile - a kernel that dropped G, the
    scaling or the clamp cannot pass the device tests' composition on any tile."""
    _, _, params, _, _ = bed_pop
    st, pv, _, _, _ = net_population()
    st, pv = st[:321], pv[:321]
    assert 0.9 <= wavenumber(2.0 * math.pi / seh.TP, sdr.DEPTH) * sdr.DEPTH <= 1.1
    for waves in (64, 11):
        worst = 1.0
        for m in seh.members(waves):
            deep = closed_loop(st, pv, params["f32"][:321], RHO, G, DT, 1, sea=m, step0=5, implicit=True)[0]["state"]
            with sdr.finite_depth_water():
                fd = closed_loop(st, pv, params["f32"][:321], RHO, G, DT, 1, sea=sdr.with_depth(m, sdr.DEPTH), step0=5, implicit=True)[0]["state"]
            for n in (65, 200, 321):
                fraction, every_tile = sdr.differs(fd, deep, n)
                assert fraction >= 0.75 and every_tile, (waves, n, fraction, every_tile)
                worst = min(worst, fraction)
        print(f"[the bottom matters, {waves} components] h = {sdr.DEPTH} m moves at least {worst:.1%} of the bodies differently from deep water, in every tile")


# ---- the recorded figures ---------------------------------------------------------------------------------------------------------
def test_recorded_isa_figures_meet_the_conditions_of_the_rung():
    """profiles/sea_depth.json (scripts/diag_sea_depth.py --isa-only): each of the 2 x 32 instantiations stays within 168 VGPRs at three
    waves per SIMD, uses no scratch, has byte for byte the LDS of the _ens kernel it is built on, and reads its table with scalar
    loads only in every one of its four component loops, the second pass with two exponentials per component."""
    import json
    isa = json.load(open(os.path.join(REPO, "profiles", "sea_depth.json")))["isa"]
    per = isa["per_instantiation"]
    assert len(per) == 64 and isa["conditions_met"] is True
    assert sum("fd_stat" in name for name in per) == 32
    for name, row in per.items():
        assert row["scratch_bytes"] == 0 and row["vgprs"] <= 168 and row["waves_per_simd"] >= 3, name
        assert row["lds_bytes"] == row["built_on_lds_bytes"] <= 54613, name
        assert row["component_loops"] == 4 and row["component_loop_scalar_loads"] > 0, name
        assert row["component_loop_lds"] == 0 and row["component_loop_vector_memory"] == 0, name
    assert isa["sample_kernel"]["scratch_bytes"] == 0
