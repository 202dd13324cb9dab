#!/usr/bin/env python3
"""Peak against statistics: the buoys of examples/irregular_sea_design_loads.py - 1 152 copies of config 1's buoy on three
lines each, nine designs of stiffness and pretension, in a JONSWAP sea of Hs 1.5 m and Tp 7 s - put through the SAME storm in
several random realisations (`--seeds`).

`track_extremes()` gives, per buoy, the largest line tension of one realisation: rerun with another seed and it moves.
`track_statistics(("z", "tension"))` gives what does not move much: the mean and the standard deviation of the tension and
the rate at which it crosses its level upwards - kept as sums inside the stepping kernel, every step, for every buoy - and
from them the most probable maximum mu + sigma * sqrt(2 ln N_up) of a storm of any length.  Per design the run prints the
spread of tension_max over the seeds beside the most probable maximum of each seed, and the number of slack-to-taut events
(up-crossings of the level 0 N) of the design's lines.

The tension's level is the mean tension of a short first run of the same realisation, so that the up-crossings are those of
the mean level; the heave's level is the draught at rest.

    python examples/mooring_response_statistics.py --steps 3600 --seeds 4
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import MooringSpread                # noqa: E402
from silver2_isaacsim_amd.sea import jonswap                          # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

LINES, RADIUS, DEPTH = 3, 15.0, 20.0                                  # the anchors: on a circle of 15 m, 20 m below the surface
STIFFNESS = (0.5, 1.0, 2.0)                                           # times MooringSpread.for_body's default
PRETENSION = (0.0, 0.1, 0.3)                                          # each line this much shorter than its reach at rest (m)
PER_DESIGN = 128
HS, TP, HEADING = 1.5, 7.0, 25.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=64, help="physics steps per kernel launch")
    ap.add_argument("--seeds", type=int, default=3, help="random realisations of the sea")
    ap.add_argument("--storm", type=float, default=3.0 * 3600.0, help="the storm the most probable maximum is asked for, s")
    args = ap.parse_args(argv)

    c1 = scenes.scene_c1()
    designs = len(STIFFNESS) * len(PRETENSION)
    n = PER_DESIGN * designs
    pr = np.tile(c1.params[:1].astype(np.float32), (n, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(n)
    st = np.zeros((n, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = 37.0 * (i % 36), 41.0 * (i // 36), z_eq, 1.0
    dt = float(np.float32(1.0 / 60.0))
    sc = scenes.Scene("mooring response statistics", st, np.zeros((n, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    centre = st[:, 0:2].astype(np.float64)
    design = i % designs
    k0, c0 = MooringSpread.for_body(mass, dt, LINES)
    k = np.repeat((k0 * np.asarray(STIFFNESS)[design // len(PRETENSION)])[:, None], LINES, axis=1)
    reach = float(np.hypot(RADIUS, DEPTH + z_eq))
    length = np.repeat((reach - np.asarray(PRETENSION)[design % len(PRETENSION)])[:, None], LINES, axis=1)
    anchors = MooringSpread.radial(LINES, RADIUS, DEPTH, centre=centre, length=length, stiffness=k, damping=c0).anchors
    storm_steps = args.storm / dt
    first = max(1, min(args.steps // 4, 600))                          # the run that finds the mean tension

    peaks, mpms, means, stds, snaps = [], [], [], [], []
    for seed in range(args.seeds):
        sea = jonswap(HS, TP, HEADING, spread="cos2", seed=seed, current=(0.4, 0.0, 0.0), g=sc.g)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.set_sea(sea)
        sim.set_mooring_spread(anchors, length=length, stiffness=k, damping=c0)
        # the slack-to-taut events of the whole run: the tension's up-crossings of 0 N (slot b); slot a is the heave
        stat = sim.track_statistics(("z", "tension"))
        sim.run_resident(first, chunk=min(args.chunk, first))
        mean_tension = stat.mean("tension")
        # from here on: the tension about its mean (slot a) and about 0 (slot b) - one record, two levels of one channel
        levels = np.stack([mean_tension, np.zeros(n)], axis=1).astype(np.float32)
        stat = sim.track_statistics(("tension", "tension"), levels=levels, reset=True)
        extremes = sim.track_extremes(from_state=False)
        sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
        rec = stat.record()
        peaks.append(extremes.tension_max())
        means.append(stat.mean("tension"))
        stds.append(stat.std("tension"))
        mpms.append(stat.most_probable_maximum("tension", steps=storm_steps))
        snaps.append((rec["up"][:, 1] & 0x7FFFFFFF).astype(np.int64))
        if not (stat.count() == args.steps).all():
            raise SystemExit("the record has not counted every step")
        sim.close()
    peaks, mpms, means, stds, snaps = (np.stack(a) for a in (peaks, mpms, means, stds, snaps))
    if not (np.isfinite(mpms).all() and np.isfinite(stds).all() and (peaks > 0.0).any()):
        raise SystemExit("a buoy's statistics are not finite, or no line ever carried load")

    print(f"{n} buoys on {LINES} lines each, {args.steps} steps ({args.steps * dt:.1f} s) per realisation, {args.seeds} realisations of JONSWAP "
          f"Hs {HS} m, Tp {TP} s; per design the median buoy; most probable maximum of a storm of {args.storm / 3600.0:.1f} h")
    for j in range(designs):
        m = design == j
        p = np.median(peaks[:, m], axis=1)
        q = np.median(mpms[:, m], axis=1)
        print(f"  stiffness {k[m][0, 0]:7.0f} N/m  pretension {PRETENSION[j % len(PRETENSION)]:4.2f} m:  spread of tension_max over {args.seeds} seeds "
              f"{p.min():8.1f} .. {p.max():8.1f} N ({100.0 * (p.max() - p.min()) / max(p.max(), 1e-30):4.1f} %)   mean {np.median(means[:, m]):8.1f} N  "
              f"sigma {np.median(stds[:, m]):7.1f} N   most probable maximum {q.min():8.1f} .. {q.max():8.1f} N   "
              f"slack-to-taut events per buoy {snaps[:, m].mean():5.2f}")
        print(f"      most probable maximum {np.median(q):.1f} N")
    return {"tension_max": peaks, "most_probable_maximum": mpms, "mean": means, "std": stds, "snaps": snaps, "design": design}


if __name__ == "__main__":
    main()
