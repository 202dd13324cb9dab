#!/usr/bin/env python3
"""Design loads over SIXTEEN REALISATIONS of the sea in ONE resident run: the 1 152 buoys of examples/irregular_sea_design_loads.py
(config 1's buoy on three lines at 120 degrees, nine designs of stiffness and pretension, 128 buoys each) once per seed of a JONSWAP
sea of Hs 1.5 m and Tp 7 s with cos^2 spreading on a 0.4 m/s current - 18 432 bodies, block m of 1 152 stepping through member m of
a `sea.SeaEnsemble` (`ClosedLoopSim.set_sea`; hydro_step_fused_tiled_multi_ens).  A design extreme is taken over realisations: the
mean of the maxima of the seeds, and their spread.  examples/mooring_response_statistics.py runs its seeds one after the other; here
they step together, and a single realisation of 1 152 buoys would leave most of the device idle.

Per design the run prints the mean and the standard deviation over the seeds of the peak line tension (per seed the median buoy's
`tension_max`), and beside them the most probable maximum of the same duration from the response statistics of section 30 - the
number that does not move with the seed.

    python examples/ensemble_design_loads.py --steps 3600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import MooringSpread                # noqa: E402
from silver2_isaacsim_amd.sea import jonswap_ensemble                 # noqa: E402
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
    ap.add_argument("--seeds", type=int, default=16, help="realisations of the sea, stepped together")
    args = ap.parse_args(argv)

    c1 = scenes.scene_c1()
    designs = len(STIFFNESS) * len(PRETENSION)
    per_sea = PER_DESIGN * designs                                    # 1 152 = 18 tiles: a member's block
    n = per_sea * args.seeds
    pr = np.tile(c1.params[:1].astype(np.float32), (n, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(n) % per_sea                                        # the same field once per member: the members differ in the sea alone
    st = np.zeros((n, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = 37.0 * (i % 36), 41.0 * (i // 36), z_eq, 1.0
    dt = float(np.float32(1.0 / 60.0))
    sc = scenes.Scene("ensemble design loads", st, np.zeros((n, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    centre = st[:, 0:2].astype(np.float64)
    design = i % designs                                              # the designs interleaved over the field
    k0, c0 = MooringSpread.for_body(mass, dt, LINES)
    k = np.repeat((k0 * np.asarray(STIFFNESS)[design // len(PRETENSION)])[:, None], LINES, axis=1)
    reach = float(np.hypot(RADIUS, DEPTH + z_eq))
    length = np.repeat((reach - np.asarray(PRETENSION)[design % len(PRETENSION)])[:, None], LINES, axis=1)
    anchors = MooringSpread.radial(LINES, RADIUS, DEPTH, centre=centre, length=length, stiffness=k, damping=c0).anchors

    ens = jonswap_ensemble(HS, TP, HEADING, seeds=range(args.seeds), bodies_per_sea=per_sea, spread="cos2", current=(0.4, 0.0, 0.0), g=sc.g)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(ens)
    sim.set_mooring_spread(anchors, length=length, stiffness=k, damping=c0)
    first = max(1, min(args.steps // 4, 600))                         # the run that finds the mean tension
    stat = sim.track_statistics(("z", "tension"))
    sim.run_resident(first, chunk=min(args.chunk, first))
    levels = np.stack([stat.mean("tension"), np.zeros(n)], axis=1).astype(np.float32)
    stat = sim.track_statistics(("tension", "tension"), levels=levels, reset=True)       # the tension about its mean, and about 0 N
    extremes = sim.track_extremes(from_state=False)
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    if not (stat.count() == args.steps).all():
        raise SystemExit("the record has not counted every step")
    peak = ens.split(extremes.tension_max())                          # seeds x bodies of a member
    mpm = ens.split(stat.most_probable_maximum("tension", steps=args.steps))
    sim.close()
    if not (np.isfinite(peak).all() and np.isfinite(mpm).all() and (peak > 0.0).any()):
        raise SystemExit("a buoy's record is not finite, or no line ever carried load")

    print(f"{args.seeds} seeds x {per_sea} buoys on {LINES} lines each = {n} bodies, {args.steps} steps ({args.steps * dt:.1f} s) in one resident run; "
          f"JONSWAP Hs {HS} m, Tp {TP} s, {len(ens.members[0].waves)} components per member; per design and seed the median buoy")
    by_design = design[:per_sea]
    means, stds = [], []
    for j in range(designs):
        m = by_design == j
        per_seed = np.median(peak[:, m], axis=1)                      # (seeds,): the design's peak tension in each realisation
        mean = float(per_seed.mean())
        std = float(per_seed.std(ddof=1)) if args.seeds > 1 else 0.0
        means.append(mean)
        stds.append(std)
        print(f"  stiffness {k[:per_sea][m][0, 0]:7.0f} N/m  pretension {PRETENSION[j % len(PRETENSION)]:4.2f} m:  mean of the maxima {mean:8.1f} N  "
              f"spread over the seeds {std:7.1f} N ({100.0 * std / max(mean, 1e-30):4.1f} %)   most probable maximum {float(np.median(mpm[:, m])):8.1f} N")
    return {"tension_max": peak, "most_probable_maximum": mpm, "mean_of_maxima": np.array(means), "std_of_maxima": np.array(stds), "design": by_design}


if __name__ == "__main__":
    main()
