"""Per-body extremes without a device (hydro_extremes_reset, hydro_step_fused_tiled_multi_ext): header, export and binding;
the marshalling of the two engine calls against the stand-in library; ClosedLoopSim picking the _ext entry under its three
runners with all 64 combinations of recorder, applied wrench, pose hold, sea, bed and lines, clear_extremes restoring the
previous calls, graph replays; the host restatement Extremes.fold by hand; the exactly rounded fp32 fma it stands on; the
tension scale and bound of the device test on the designed population; and one physical case, the moored buoy in a current.

The device tests are tests/test_extremes_gpu.py."""
import ctypes
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import extremes_reference as er
import mooring_reference as mr
from closed_loop_reference import closed_loop
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd import scenes, simulate
from silver2_isaacsim_amd.extremes import Extremes
from silver2_isaacsim_amd.mooring import Mooring
from silver2_isaacsim_amd.sea import SeaState
from engine_stand_ins import BODIES, eng, ext_sim as _sim, FUSED_HEAD, H, KE, lib, N, P13, refused, S, SO, STREAM, T, TILES, _without_extremes  # noqa: F401  (fixtures are requested by name)
from mooring_population import buoy, DEPTH, designed_population, TIES

ENTRIES = ("hydro_extremes_reset", "hydro_step_fused_tiled_multi_ext")
A = T((TILES, 6, 64), 0x88000000)
C = T((TILES, 17, 64), 0x90000000)
M = T((TILES, 9, 64), 0xA0000000)
E = T((TILES, 8, 64), 0xA8000000)                                 # the extremes record
INF = np.float32(np.inf)


# ---- C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entries():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code) and name in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert "hydro_extremes_reset, hydro_step_fused_tiled_multi_ext" in text.split("#define HYDRO_VERSION")[0]    # the version comment
    assert int(re.search(r"#define HYDRO_EXT_FIELDS\s+(\d+)", code).group(1)) == nat.EXT_FIELDS == ex.FIELDS == len(ex.NAMES) == 8
    assert ex.NAMES == ("x_min", "x_max", "y_min", "y_max", "z_min", "z_max", "speed2_max", "tension_max")
    assert [ex.INDEX[k] for k in ex.NAMES] == list(range(8)) and (ex.X_MIN, ex.Z_MAX, ex.SPEED2_MAX, ex.TENSION_MAX) == (0, 5, 6, 7)
    # the mooring entry's argument list with `extremes`, `extremes_tile_stride` in front of step0
    moor, ext = (nat.SIGNATURES["hydro_step_fused_tiled_multi_" + k][1] for k in ("moor", "ext"))
    assert ext == moor[:-2] + [ctypes.c_void_p, ctypes.c_int64] + moor[-2:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    tail = "int64_t step0, void *stream"
    assert proto("hydro_step_fused_tiled_multi_ext") == (proto("hydro_step_fused_tiled_multi_moor")[:-len(tail)]
                                                         + "float *extremes, int64_t extremes_tile_stride, " + tail)
    assert proto("hydro_extremes_reset") == ("hydro_t *h, int64_t n, const float *state, int64_t state_tile_stride, float *extremes, "
                                             "int64_t extremes_tile_stride, void *stream")
    # the header fixes the record, when it is read and written, the sample, the update and what is not provided
    for phrase in ("x_min x_max | y_min y_max | z_min z_max | speed2_max | tension_max", "extremes_tile_stride >= 512",
                   "READ AT THE START OF A LAUNCH AND\n * WRITTEN AT ITS END", "fma(v_z, v_z, fma(v_y, v_y, v_x * v_x))",
                   "m = (x < m) ? x : m            M = (x > M) ? x : M", "never fminf / fmaxf", "a NaN sample never enters",
                   "a NaN accumulator stays NaN", "+0 against -0 included", "Lanes >= n of the last tile are never written",
                   "means and variances", "the step at which an extreme occurred", "the extremes of the launch's INITIAL state",
                   "extremes of the wrench", "[+inf, -inf, +inf, -inf, +inf, -inf, +0, +0]", "a replay accumulates"):
        assert phrase in text, phrase


def test_library_exports_the_entries(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib_ = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", out, re.M) and hasattr(lib_, name)


def test_null_handle_gives_e_arg_without_a_device(native_built):
    lib_ = nat.load()
    written = ctypes.c_int64(-7)
    rc = lib_.hydro_step_fused_tiled_multi_ext(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                               None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), None, 384, 0, None, 1088, None, 576,
                                               None, 512, 0, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7
    assert lib_.hydro_extremes_reset(None, 64, None, 832, None, 512, None) == -1


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_extremes_reset(lib, eng):
    assert eng.extremes_reset(E, N, stream=STREAM) is E
    assert eng.extremes_reset(E, N, S, stream=STREAM) is E
    assert lib.calls == [("hydro_extremes_reset", (H, 1000, None, 0, 0xA8000000, 512, STREAM)),
                         ("hydro_extremes_reset", (H, 1000, 0x10000000, 832, 0xA8000000, 512, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 8, 64) tensor on cuda:0", eng.extremes_reset, M, N, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.extremes_reset, E, N, A, stream=STREAM)


def test_step_fused_tiled_multi_ext(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    line, record = (0xA0000000, 576), (0xA8000000, 512)
    cases = [(E, dict(mooring=M), None, 0, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, None, 0) + line + record + (0, STREAM)),
             (E, dict(mooring=M, control=C, applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO, 123456789012,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0, 0x90000000, 1088) + line + record
              + (123456789012, STREAM)),
             # extremes alone: no lines, NULL and stride 0 in their place, `extremes` in front of step0
             (E, dict(applied=A, log=log, every=4, phase=2, row0=3), None, 5,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1, None, 0) + (None, 0) + record + (5, STREAM)),
             # no record: NULL and stride 0, and the library dispatches to the mooring entry's launch
             (None, dict(mooring=M, control=C), None, 9,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1, 0x90000000, 1088) + line + (None, 0) + (9, STREAM))]
    for extremes, kw, state_out, step0, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_ext(S, P13, N, 0.01, 7, step0, extremes, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [("hydro_step_fused_tiled_multi_ext", want)]
    lib.calls.clear()
    refused(lib, "frame must be 'world' or 'body'", eng.step_fused_tiled_multi_ext, S, P13, N, 0.01, 3, 0, E, M, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 8, 64) tensor on cuda:0", eng.step_fused_tiled_multi_ext, S, P13, N, 0.01, 3, 0, M, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 9, 64) tensor on cuda:0", eng.step_fused_tiled_multi_ext, S, P13, N, 0.01, 3, 0, E, E, stream=STREAM)


# ---- ClosedLoopSim's bookkeeping -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("run", ["eager", "replay_sized_run", "resident"])
@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=6)),
                         ids=lambda c: "".join(n for n, on in zip(("rec", "App", "Ctl", "Sea", "Bed", "Moor"), c) if on) or "plain")
def test_the_extremes_entry_is_picked_with_every_combination_and_cleared_again(monkeypatch, combo, run):
    recorder, applied, control, sea, bed, lines = combo
    s = _sim(monkeypatch, *combo)
    assert simulate.ClosedLoopSim.extremes is None and s.extremes is None       # a class default: a sim tracks nothing until asked
    go = {"eager": lambda: s.run_eager(3), "replay_sized_run": lambda: s.run(3, graph_steps=0), "resident": lambda: s.run_resident(5, chunk=2)}[run]
    steps = [2, 2, 1] if run == "resident" else [1, 1, 1]
    go()
    before = [c["method"] for c in s.engine.calls]
    assert before == [_without_extremes(*combo, eager=run != "resident")] * 3
    s.engine.calls.clear()
    s.steps_done = 0
    view = s.track_extremes()
    assert view is s.extremes and isinstance(view, Extremes) and tuple(view.buffer.shape) == (2, 8, 64)
    assert s.engine.calls == [("extremes_reset", view.buffer, BODIES, s.cur)]   # seeded from the current state
    s.engine.calls.clear()
    go()
    done = 0
    assert len(s.engine.calls) == 3
    for i, (call, k) in enumerate(zip(s.engine.calls, steps)):
        assert call["method"] == "ext" and call["steps"] == k and call["step0"] == done and call["extremes"] is view.buffer
        assert call["mooring"] is s.mooring and (s.mooring is not None) == lines
        assert call["control"] is s.control and call["applied"] is s.applied and call["frame"] == "world"
        assert call["log"] is (s.recorder.log if recorder else None)
        assert call["cur"] == ("buffer B", "buffer A")[i % 2]      # (three steps were taken before the extremes were tracked)
        done += k
    assert s.steps_done == done
    s.engine.calls.clear()
    s.clear_extremes()
    assert s.extremes is None and s.engine.calls == []
    go()
    assert [c["method"] for c in s.engine.calls] == before         # every call is again the one the sim made before
    s.clear_extremes()                                             # a second clear is nothing
    assert len(s.engine.calls) == 3
    s.engine.calls.clear()
    again = s.track_extremes(from_state=False)
    assert again is view and again.buffer is view.buffer           # the view and the buffer's address never change
    assert s.engine.calls == [("extremes_reset", view.buffer, BODIES, None)]
    s.engine.calls.clear()
    view.reset()
    assert s.engine.calls == [("extremes_reset", view.buffer, BODIES, s.cur)]


def test_graph_replays_take_extremes_and_still_refuse_lines_with_waves(monkeypatch):
    captured = []
    monkeypatch.setattr(simulate.ClosedLoopSim, "_capture", lambda self, k: captured.append(k) or setattr(self, "_graph", None))
    s = _sim(monkeypatch, lines=True)
    s._graph = "a captured graph without extremes"
    s.track_extremes()
    assert s._graph is None                                      # captured launches are of another entry
    s._graph = "a captured graph with extremes"
    s.track_extremes()
    assert s._graph == "a captured graph with extremes"         # a reset, the same entry and buffer: the capture stands
    s._graph = None
    s.sea = SeaState((0.3, 0.0, 0.0))
    with pytest.raises(AttributeError):                          # gets as far as replaying the (faked) capture
        s.run(64, graph_steps=32)
    assert captured == [32]
    s.sea = SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError, match="a sea with waves cannot ride in graph replays"):
        s.run(64, graph_steps=32)
    assert captured == [32] and s.steps_done == 0
    s._graph = "a captured graph with extremes"
    s.clear_extremes()
    assert s._graph is None
    s.fused = False
    with pytest.raises(ValueError, match="fused"):
        s.track_extremes()


# ---- the host restatement ------------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(v: Fraction) -> np.float32:
    """Round-to-nearest-even of an exact rational to fp32 (normal range), in integers."""
    if v == 0:
        return np.float32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    scaled = v / Fraction(2) ** (e - 23)                         # in [2^23, 2^24)
    q, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and q & 1):
        q += 1
    return np.float32(sign * float(q) * 2.0 ** (e - 23))


def test_fma32_is_rounded_once():
    """extremes.fma32 against exact rational arithmetic rounded once to fp32: random operands, operands built so that the fp64
    sum lands on a tie of the fp32 grid (where rounding twice goes wrong), and the kernel's speed2 chain."""
    rng = np.random.default_rng(11)
    a = rng.normal(size=4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, 4000).astype(np.float32)
    b = rng.normal(size=4000).astype(np.float32)
    c = (rng.normal(size=4000) * np.abs(a.astype(np.float64) * b)).astype(np.float32)
    # ties: a * b = 1 + 2^-24 exactly half way between two floats would need 25 bits; a = 1 + 2^-12, b = 1 + 2^-12 gives
    # 1 + 2^-11 + 2^-24: with c = 2^-60 the exact sum is just above the half-way point, the fp64 sum ON it
    ta = np.full(4, 1.0 + 2.0 ** -12, np.float32)
    tb = ta.copy()
    tc = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -70, -2.0 ** -70], np.float32)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = ex.fma32(a, b, c)
    want = np.array([_round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (twice[-4:] != want[-4:]).any()                       # the ties are where the double rounding differs
    v = rng.normal(size=(500, 3)).astype(np.float32)
    s2 = ex.speed2(v)
    for row, got_row in zip(v, s2):
        p = np.float32(row[0] * row[0])
        p = _round_fraction_to_f32(Fraction(float(row[1])) ** 2 + Fraction(float(p)))
        assert got_row == _round_fraction_to_f32(Fraction(float(row[2])) ** 2 + Fraction(float(p)))


def _states(rows):
    """(rows, 1, 13) states from (x, y, z, vx, vy, vz) rows."""
    st = np.zeros((len(rows), 1, 13), np.float32)
    for j, r in enumerate(rows):
        st[j, 0, 0:3], st[j, 0, 7:10], st[j, 0, 6] = r[0:3], r[3:6], 1.0
    return st


def test_fold_by_hand():
    st = _states([(1.0, -2.0, -5.0, 3.0, 0.0, 4.0), (0.5, -1.0, -6.0, 0.0, 1.0, 0.0), (2.0, -3.0, -5.5, 1.0, 2.0, 2.0)])
    T_ = np.array([[10.0], [0.0], [12.5]], np.float32)
    rec = Extremes.fold(st, T_)
    assert rec.dtype == np.float32 and rec.shape == (1, 8)
    assert rec[0].tolist() == [0.5, 2.0, -3.0, -1.0, -6.0, -5.0, 25.0, 12.5]
    # no sample: the empty record; one body more: independent columns
    assert np.array_equal(Extremes.fold(st[:0], T_[:0]), Extremes.empty(1)) and Extremes.empty(2).tolist() == [[INF, -INF, INF, -INF, INF, -INF, 0.0, 0.0]] * 2
    # a seed counts as what came before: the larger box of the two, the larger maxima
    seed = np.array([[0.75, 9.0, -2.5, -2.5, -7.0, -7.0, 30.0, 11.0]], np.float32)
    assert Extremes.fold(st, T_, seed)[0].tolist() == [0.5, 9.0, -3.0, -1.0, -7.0, -5.0, 30.0, 12.5]
    assert seed[0, 0] == 0.75                                    # the seed is not written
    # the seed of a state: min = max = p, speed2 of its v, tension +0
    s0 = ex.seed_of(st[0])
    assert s0[0].tolist() == [1.0, 1.0, -2.0, -2.0, -5.0, -5.0, 25.0, 0.0] and not np.signbit(s0[0, 7])
    assert np.array_equal(Extremes.fold(st[1:], T_[1:], s0), Extremes.fold(st, np.array([[0.0], [0.0], [12.5]], np.float32)))
    # folding in two parts is folding at once
    assert np.array_equal(Extremes.fold(st[2:], T_[2:], Extremes.fold(st[:2], T_[:2])), rec)
    with pytest.raises(ValueError):
        Extremes.fold(st, T_[:2])
    with pytest.raises(ValueError):
        Extremes.fold(st, T_, seed[:, :7])


def test_fold_nan_and_signed_zero():
    nan = np.float32(np.nan)
    # a NaN sample is ignored: in every field
    st = _states([(1.0, 1.0, 1.0, 1.0, 0.0, 0.0), (nan, nan, nan, nan, 0.0, 0.0), (2.0, 0.0, 1.0, 0.0, 0.0, 0.0)])
    rec = Extremes.fold(st, np.array([[1.0], [nan], [0.5]], np.float32))
    assert rec[0].tolist() == [1.0, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # a NaN accumulator is kept
    seed = np.full((1, 8), nan, np.float32)
    assert np.isnan(Extremes.fold(st, np.ones((3, 1), np.float32), seed)).all()
    seed = Extremes.empty(1)
    seed[0, ex.X_MAX] = seed[0, ex.TENSION_MAX] = nan
    rec = Extremes.fold(st, np.ones((3, 1), np.float32), seed)
    assert np.isnan(rec[0, [ex.X_MAX, ex.TENSION_MAX]]).all() and rec[0, ex.X_MIN] == 1.0 and rec[0, ex.SPEED2_MAX] == 1.0
    # -0 against +0 keeps the first, whichever it is: an equal value leaves the accumulator's bits
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        st = _states([(first, first, first, 0.0, 0.0, 0.0), (second, second, second, 0.0, 0.0, 0.0)])
        rec = Extremes.fold(st, np.array([[first], [second]], np.float32), None)
        want = np.signbit(np.float32(first))
        assert (np.signbit(rec[0, 0:6]) == want).all() and not rec[0, 0:6].any()
    rec = Extremes.fold(_states([(0, 0, 0, 0, 0, 0)]), np.array([[-0.0]], np.float32))
    assert not np.signbit(rec[0, ex.TENSION_MAX])                # the empty record's +0 stays against a -0 sample


def test_excursion_is_the_farthest_corner_of_the_box():
    rec = np.array([[-1.0, 3.0, -4.0, 2.0, -9.0, -8.0, 0.0, 0.0], [5.0, 5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    assert ex.excursion(rec, (0.0, 0.0)).tolist() == [5.0, pytest.approx(np.hypot(5.0, 5.0))]
    assert ex.excursion(rec, [[3.0, 2.0], [5.0, 5.0]]).tolist() == [pytest.approx(np.hypot(4.0, 6.0)), 0.0]
    assert np.isnan(ex.excursion(Extremes.empty(1), (0.0, 0.0))).all()          # nothing sampled yet


def test_the_view_reads_the_tiled_record(monkeypatch):
    s = _sim(monkeypatch)
    view = s.track_extremes(from_state=False)
    rows = np.arange(BODIES * 8, dtype=np.float32).reshape(BODIES, 8)
    view.buffer.copy_(torch.from_numpy(scenes.to_tiled(rows)))
    assert np.array_equal(view.bodies(), rows) and view.n == BODIES
    for j, name in enumerate(ex.NAMES):
        assert np.array_equal(getattr(view, name)(), rows[:, j]) and np.array_equal(view.field(name), rows[:, j])
    assert np.allclose(view.speed_max(), np.sqrt(rows[:, 6].astype(np.float64)))
    assert np.array_equal(view.excursion((0.0, 0.0)), ex.excursion(rows, (0.0, 0.0)))


# ---- the tension of the device test: its scale and its bound, on the host ------------------------------------------------------------
def test_the_tension_bound_on_the_designed_population():
    """The header's fp32 order (mooring_reference._fp32_terms) against mooring_reference.tension over the designed population,
    the ties aside, in units of 2^-24 of extremes_reference.tension_scale = k (l^ + L0) + c u^: TENSION_BOUND is the next power
    of two at or above twice the largest."""
    st, _, _, rec = designed_population()
    off = ~np.isin(np.arange(321), TIES)
    on = mr.taut_fp32(rec, st)
    T32 = er.tension_fp32_emulated(rec, st)
    ref = mr.tension(rec, st, on)
    live = (ref > 0) & off
    assert live.mean() >= 0.25 and not T32[~live & off].any()
    err = np.abs(T32[live].astype(np.float64) - ref[live]) / (mr.ULP * er.tension_scale(rec, st)[live])
    print(f"[extremes, designed population, fp32 order emulated on the host] tension {err.max():.3f} units of 2^-24 of the scale "
          f"(bound {er.TENSION_BOUND:g})")
    assert er.TENSION_BOUND == 2.0 ** np.ceil(np.log2(2.0 * err.max()))
    assert (er.tension_scale(rec, st)[live] >= ref[live]).all()


# ---- the physics: config 1's buoy on a line in a current ------------------------------------------------------------------------------
def test_the_buoy_in_a_current_its_peak_tension_and_its_reach():
    st, pv, pr, sc, dt, z_eq, mass = buoy()
    k, c = Mooring.for_body(mass, dt)
    lines = Mooring((0.0, 0.0, z_eq - DEPTH), length=DEPTH + 0.5, stiffness=k, damping=c)
    run = closed_loop(st, pv, pr, sc.rho, sc.g, dt, 900, moor=lines.record, sea=SeaState((0.5, 0.0, 0.0)), implicit=True)
    states = np.stack([r["state"] for r in run])                 # (900, 1, 13): the state each step produced
    tensions = np.stack([r["tension"] for r in run])             # (900, 1): the T formed IN that step
    rec = Extremes.fold(states, tensions, ex.seed_of(st))
    per_step = np.array([float(mr.tension(lines.record, r["input"])[0]) for r in run])
    assert (rec[0, ex.TENSION_MAX] >= per_step.astype(np.float32)).all() and rec[0, ex.TENSION_MAX] == np.float32(per_step.max()) > 0
    xs = np.concatenate([st[:, 0], states[:, 0, 0]])
    assert rec[0, ex.X_MAX] == xs.max() > 1.0 and rec[0, ex.X_MIN] == xs.min() == 0.0
    zs = np.concatenate([st[:, 2], states[:, 0, 2]])
    assert rec[0, ex.Z_MAX] == zs.max() >= np.float32(z_eq) and rec[0, ex.Z_MIN] == zs.min() < np.float32(z_eq)   # the line pulls it down from where it floated
    reach = ex.excursion(rec, (0.0, 0.0))[0]
    print(f"[buoy in a current] peak tension {rec[0, ex.TENSION_MAX]:.1f} N  watch circle {reach:.3f} m  z {rec[0, ex.Z_MIN]:+.3f} .. {rec[0, ex.Z_MAX]:+.3f} m  "
          f"top speed {np.sqrt(rec[0, ex.SPEED2_MAX]):.3f} m/s")
    assert reach == pytest.approx(float(xs.max()), abs=1e-6) and 0.0 < np.sqrt(rec[0, ex.SPEED2_MAX]) < 1.0
