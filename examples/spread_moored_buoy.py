#!/usr/bin/env python3
"""A spread mooring: config 1's buoy (a floating unit cube, 500 kg) on THREE lines at 120 degrees to anchors 20 m down, in 64
copies that meet a 0.5 m/s current from 64 different headings - and, beside them, the same 64 buoys on ONE line each.  A
single line gives a watch circle: the buoy swings to wherever the current pushes it.  The spread keeps it on station
whatever the heading.  `ClosedLoopSim.track_extremes()` keeps, inside the stepping kernel, the box each buoy stayed in and
the largest tension any of its lines carried (`tension_max`): what sizes the lines.

The sea is the scene's (one current for all bodies), so a copy's heading is set by turning its spread and the buoy against
the current.

    python examples/spread_moored_buoy.py --steps 3600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import Mooring, MooringSpread       # noqa: E402
from silver2_isaacsim_amd.sea import SeaState                         # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

COPIES, LINES = 64, 3
RADIUS, DEPTH = 15.0, 20.0                                            # the anchors: on a circle of 15 m, 20 m below the surface
PRETENSION = 0.1                                                      # each line this much shorter than its reach at rest (m)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=64, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    c1 = scenes.scene_c1()
    pr = np.tile(c1.params[:1].astype(np.float32), (COPIES, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(COPIES)
    heading = 2.0 * np.pi * i / COPIES                                # where the current comes from, seen from the spread
    st = np.zeros((COPIES, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2] = 50.0 * (i % 8), 50.0 * (i // 8), z_eq
    st[:, 5], st[:, 6] = np.sin(-0.5 * heading), np.cos(-0.5 * heading)
    dt = float(np.float32(1.0 / 60.0))
    sc = scenes.Scene("spread moored buoys", st, np.zeros((COPIES, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    centre = st[:, 0:2].astype(np.float64)
    current = SeaState((0.5, 0.0, 0.0))

    k, c = MooringSpread.for_body(mass, dt, LINES)
    reach = float(np.hypot(RADIUS, DEPTH + z_eq))
    lines = MooringSpread.radial(LINES, RADIUS, DEPTH, centre=centre, length=reach - PRETENSION, stiffness=k, damping=c)
    # turn each copy's spread against the current: radial() takes one heading, so the anchors are turned about their centres here
    a = lines.record.reshape(COPIES, LINES, 9)[:, :, 0:3].copy()
    d = a[:, :, 0:2] - centre[:, None, :]
    cos, sin = np.cos(-heading)[:, None], np.sin(-heading)[:, None]
    a[:, :, 0], a[:, :, 1] = centre[:, None, 0] + cos * d[:, :, 0] - sin * d[:, :, 1], centre[:, None, 1] + sin * d[:, :, 0] + cos * d[:, :, 1]

    spread = ClosedLoopSim(sc, implicit_drag=True)
    spread.set_sea(current)
    spread.set_mooring_spread(a, length=reach - PRETENSION, stiffness=k, damping=c)
    on_three = spread.track_extremes()
    spread.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    excursion, peak = on_three.excursion(centre), on_three.tension_max()
    spread.close()

    k1, c1_ = Mooring.for_body(mass, dt)
    single = ClosedLoopSim(sc, implicit_drag=True)
    single.set_sea(current)
    single.set_mooring(np.concatenate([centre, np.full((COPIES, 1), -DEPTH)], axis=1), length=DEPTH + z_eq + 0.5, stiffness=k1, damping=c1_)
    on_one = single.track_extremes()
    single.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    circle, peak_one = on_one.excursion(centre), on_one.tension_max()
    single.close()

    print(f"{COPIES} buoys, {args.steps} steps ({args.steps * dt:.1f} s), 0.5 m/s current; per heading of the current (degrees):")
    print("  heading   excursion on three lines m   watch circle on one line m   tension_max N (spread)   (one line)")
    for j in range(0, COPIES, 8):
        print(f"  {np.degrees(heading[j]):7.1f}   {excursion[j]:26.3f}   {circle[j]:27.3f}   {peak[j]:22.1f}   {peak_one[j]:10.1f}")
    print(f"largest excursion on three lines {excursion.max():.3f} m, on one line {circle.max():.3f} m")
    print("tension_max (N): " + " ".join(f"{t:.1f}" for t in peak[::8]))
    if not (peak > 0.0).all():
        raise SystemExit("a spread never carried load")
    if not excursion.max() < circle.max():
        raise SystemExit("the spread did not hold the buoys better than one line")
    return {"excursion": excursion, "watch_circle": circle, "tension_max": peak}


if __name__ == "__main__":
    main()
