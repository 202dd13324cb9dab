"""What the sea-ensemble tests share (tests/test_sea_ensemble.py, tests/test_sea_ensemble_gpu.py): the "ens" row of the resident
harness, one caller of the engine entry and one of the C entry, the members, and the condition that makes the identity of
include/hydro.h ("Sea ensemble") mean something - any two members move nearly every body differently.

Importing this module registers `"ens"` in resident_harness.ENTRIES and RAW_EXTRAS: the signature is the _stat entry's.  `step`'s
defaults name only "spread", "irr" and "stat", so `launch` passes the counts and the channels explicitly.

THE MEMBERS: six JONSWAP seas (n = 321 at tiles_per_sea = 1 needs six) that differ in seed, heading and current, Hs 0.8 .. 1.8 m,
Tp 7 s, cos^2 spreading, 11 or 64 components.  The currents differ by 0.15 m/s or more in x or y between any two members, so the
drag on every wetted body differs by far more than an fp32 rounding after one step: `apart` below checks it, on the fp64 closed
loop in the CPU module and on the parent entry's own runs in the GPU module.
"""
import numpy as np

import resident_harness as rh
from silver2_isaacsim_amd.sea import SeaEnsemble, jonswap

rh.ENTRIES["ens"] = ("step_fused_tiled_multi_ens", rh.ENTRIES["stat"][1])
rh.RAW_EXTRAS["ens"] = rh.RAW_EXTRAS["stat"]

SEEDS = (11, 12, 13, 14, 15, 16)
HEADINGS = (0.0, 40.0, 95.0, 150.0, 220.0, 300.0)
CURRENTS = ((0.5, -0.2, 0.05), (-0.3, 0.4, 0.0), (0.2, 0.6, -0.05), (-0.6, -0.1, 0.0), (0.0, -0.5, 0.05), (0.35, 0.15, 0.0))
HS = (0.8, 1.0, 1.2, 1.4, 1.6, 1.8)
TP = 7.0


def members(waves: int, count: int = 6):
    """The first `count` members with `waves` components each."""
    return [jonswap(HS[m], TP, HEADINGS[m], components=waves, seed=SEEDS[m], spread="cos2", current=CURRENTS[m]) for m in range(count)]


def ensemble(waves: int, n: int, tiles_per_sea: int) -> SeaEnsemble:
    """Exactly the members a launch of n bodies needs at `tiles_per_sea`."""
    tiles = (n + 63) // 64
    return SeaEnsemble(members(waves, -(-tiles // tiles_per_sea)), 64 * tiles_per_sea)


def apart(states, n: int):
    """`states`: one (n, 13) fp32 state after one step per member, every member over the WHOLE population.  For every pair of members:
    (the smallest fraction of bodies whose state differs in some bit, whether some body differs in EVERY tile)."""
    worst, every_tile = 1.0, True
    for a in range(len(states)):
        for b in range(a + 1, len(states)):
            differs = (np.asarray(states[a][:n], np.float32).view(np.uint32) != np.asarray(states[b][:n], np.float32).view(np.uint32)).any(axis=1)
            worst = min(worst, float(differs.mean()))
            every_tile = every_tile and all(differs[t:t + 64].any() for t in range(0, n, 64))
    return worst, every_tile


def launch(eng, cur, old, n, steps, *, step0=0, statistics=None, levels=None, channels=(2, 6), spread=None, layers=1, tether=None, net_layers=1,
           peaks=None, extremes=None, applied=None, frame="world", control=None, implicit=False, ke=None, dt=rh.DT, entry="ens", **kw):
    """One launch of the _ens entry (or, entry="stat", of the parent's) through the harness's one engine caller: (state, prev_out)."""
    return rh.step(eng, entry, cur, old, n, steps, step0=step0, applied=applied, frame=frame, control=control, mooring=spread, extremes=extremes,
                   tether=tether, layers=net_layers, peaks=peaks, mooring_layers=layers, statistics=statistics, levels=levels, channels=tuple(channels),
                   implicit=implicit, ke=ke, dt=dt, **kw)


def raw_ens(eng, n, state, prev, out, pvo, *, entry="ens", steps=1, step0=0, implicit=0, log=None, applied=None, s_applied=0, control=None, s_control=0,
            mooring=None, s_mooring=0, layers=1, extremes=None, s_extremes=0, tether=None, s_tether=0, net_layers=1, peaks=None, s_peaks=0,
            statistics=None, s_statistics=0, levels=None, s_levels=0, channels=(2, 6)):
    """hydro_step_fused_tiled_multi_ens with the guard tests' strides on state, prev, out and pvo.  Returns (rc, rows_written from -7)."""
    return rh.raw(eng, entry, n, state, prev, out, pvo, steps=steps, step0=step0, implicit=implicit, log=log, applied=applied, s_applied=s_applied,
                  control=control, s_control=s_control, mooring=mooring, s_mooring=s_mooring, mooring_layers=layers, extremes=extremes, s_extremes=s_extremes,
                  tether=tether, s_tether=s_tether, tether_layers=net_layers, peaks=peaks, s_peaks=s_peaks, statistics=statistics, s_statistics=s_statistics,
                  levels=levels, s_levels=s_levels, channels=channels)
