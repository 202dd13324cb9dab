"""What the statistics tests share (tests/test_statistics.py, tests/test_statistics_gpu.py): bitwise comparison of records, the
guard layout of the statistics record, one caller of the engine entry and one of the C entry, and the scene of the up-crossing
test - config 1's buoy, copied along x, in a regular wave whose period is a few steps.

No device is needed to import this module; the callers that launch take the engine and the tensors they are given.
"""
import math

import numpy as np

import closed_loop_reference as clr
from mooring_population import buoy
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.sea import SeaState

S_ST = 11 * 64 + 36                                               # the statistics record's tile stride in the guard tests (4-byte units)
S_LV = 2 * 64 + 20                                                # the level record's
NAN_BITS = np.uint32(0x7FC00000)


def same_record(a, b, nan_equal=True) -> bool:
    """Two host records (statistics.empty's dict) bit for bit; a NaN sum equals a NaN sum whatever its payload."""
    sa, sb = np.ascontiguousarray(a["sums"], np.float64), np.ascontiguousarray(b["sums"], np.float64)
    same = sa.view(np.uint64) == sb.view(np.uint64)
    if nan_equal:
        same |= np.isnan(sa) & np.isnan(sb)
    return bool(same.all()) and np.array_equal(np.asarray(a["up"], np.uint32), np.asarray(b["up"], np.uint32)) \
        and np.array_equal(np.asarray(a["n"], np.uint32), np.asarray(b["n"], np.uint32))


def live_words(n: int, stride: int = S_ST) -> np.ndarray:
    """(tiles, stride) bool: the 4-byte words of a guarded statistics buffer that belong to bodies 0 .. n - 1."""
    tiles = (n + 63) // 64
    live = np.zeros((tiles, stride), bool)
    body = np.arange(tiles * 64).reshape(tiles, 64) < n          # (tile, lane)
    for j in range(4):
        for half in range(2):
            live[:, j * 128 + half:j * 128 + 128:2] = body
    for w in range(3):
        live[:, 512 + w * 64:512 + (w + 1) * 64] = body
    return live


def unguard(flat_words, n: int, stride: int = S_ST):
    """A guarded statistics buffer as host uint32 words -> (the record of bodies 0 .. n - 1, every other word: must still be NaN_BITS)."""
    host = np.asarray(flat_words, np.uint32).reshape(-1, stride)
    rec = stx.unpack(np.ascontiguousarray(host[:, :704]).view(np.float32).reshape(-1, 11, 64), n)
    return rec, host[~live_words(n, stride)]


def launch(eng, cur, old, n, dt, steps, *, step0=0, statistics=None, levels=None, channels=(2, 6), spread=None, layers=1, tether=None, net_layers=1,
           peaks=None, extremes=None, applied=None, frame="world", control=None, implicit=False, ke=None, **kw):
    """One launch of the _stat entry through the engine: (state, prev_out)."""
    eng.step_fused_tiled_multi_stat(cur, old, n, dt, steps, step0, statistics, levels, channels[0], channels[1], spread, layers, tether, net_layers,
                                    peaks, extremes, control, applied, frame, implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def raw_stat(eng, n, dt, state, prev, out, pvo, strides, *, steps=1, step0=0, implicit=0, log=None, applied=None, s_applied=0, control=None, s_control=0,
             mooring=None, s_mooring=0, layers=1, extremes=None, s_extremes=0, tether=None, s_tether=0, net_layers=1, peaks=None, s_peaks=0,
             statistics=None, s_statistics=S_ST, levels=None, s_levels=S_LV, channels=(2, 6)):
    """hydro_step_fused_tiled_multi_stat; `strides` = (state, prev, out, pvo).  Returns (rc, rows_written from the sentinel -7)."""
    import resident_harness as rh                                  # (imports torch: only the callers that launch come here)
    assert tuple(strides) == (rh.S_IN, rh.S_PV, rh.S_OUT, rh.S_PVO) and dt == rh.DT
    return rh.raw(eng, "stat", n, state, prev, out, pvo, steps=steps, step0=step0, implicit=implicit, log=log, applied=applied, s_applied=s_applied,
                  control=control, s_control=s_control, mooring=mooring, s_mooring=s_mooring, mooring_layers=layers, extremes=extremes, s_extremes=s_extremes,
                  tether=tether, s_tether=s_tether, tether_layers=net_layers, peaks=peaks, s_peaks=s_peaks, statistics=statistics, s_statistics=s_statistics,
                  levels=levels, s_levels=s_levels, channels=channels)


# ---- the scene in which up-crossings really occur ------------------------------------------------------------------------------------------
CROSS_STEPS = 24                                                  # the launch
CROSS_PERIOD = 6                                                  # the wave's period, in steps


def crossing_scene(n: int):
    """(state, prev, params, scene, dt, sea): n copies of config 1's buoy at rest at its draught, 0.9 m apart along x, in a regular
    wave of amplitude 0.15 m and a wavelength of 7.3 m whose period is CROSS_PERIOD steps (omega is taken as given: the model does
    not tie it to the wavelength), so that the copies meet it at phases of their own and heave at that period."""
    st, pv, pr, sc, dt, _, _ = buoy()
    st, pv, pr = np.tile(st, (n, 1)), np.tile(pv, (n, 1)), np.tile(pr, (n, 1))
    st[:, 0] = np.float32(0.9) * np.arange(n, dtype=np.float32)
    sea = SeaState((0.0, 0.0, 0.0))
    sea.add_wave(0.15, 2.0 * math.pi / 7.3, 0.0, 2.0 * math.pi / (CROSS_PERIOD * dt), 0.4)
    return st, pv, pr, sc, dt, sea


def crossing_reference(n: int, implicit: bool = True):
    """The fp64 closed loop over the crossing scene: ((steps, n, 13) fp32 states after every step, (n, 2) fp32 levels - the mean of
    the recorded vz and z - and the record `fold` gives for channels (vz, z) about them)."""
    st, pv, pr, sc, dt, sea = crossing_scene(n)
    steps = clr.closed_loop(st, pv, pr, sc.rho, sc.g, dt, CROSS_STEPS, sea=sea, implicit=implicit)
    states = np.stack([np.asarray(s["state"], np.float32) for s in steps])
    levels = levels_of(states)
    return states, levels, stx.fold(None, states[:, :, 9], states[:, :, 2], levels)


def levels_of(states) -> np.ndarray:
    """(n, 2) fp32: the mean over the rows of vz and of z, in fp64, rounded once."""
    s = np.asarray(states, np.float64)
    return np.stack([s[:, :, 9].mean(axis=0), s[:, :, 2].mean(axis=0)], axis=1).astype(np.float32)
