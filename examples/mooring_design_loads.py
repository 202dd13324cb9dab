#!/usr/bin/env python3
"""Design loads of a mooring, by brute force: 4 608 copies of config 1's buoy (a floating unit cube, 500 kg), each on a line
of its own to a bed 20 m down, in a 0.5 m/s current and two regular wave trains.  The copies differ in what a designer
varies - the line's stiffness (three values) and its length (three values), nine design classes - and in where they float
and how they are turned, so each meets the waves at a phase of its own.  ONE resident run carries all of them through the
storm; `ClosedLoopSim.track_extremes()` keeps, inside the stepping kernel, each buoy's peak line tension and the box it
stayed in: eight floats per body are read back at the end, no trajectory is recorded.

The sea is the scene's: every buoy meets the same two wave periods (a sea state is set per scene, not per body).  To vary
the period, run the scene once per sea.

    python examples/mooring_design_loads.py --steps 3600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import Mooring                      # noqa: E402
from silver2_isaacsim_amd.sea import SeaState                         # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

DEPTH = 20.0                                                          # the anchors below the buoys' equilibrium position (m)
STIFFNESS = (0.5, 1.0, 2.0)                                           # times Mooring.for_body's default
SLACK = (-0.1, 0.25, 1.0)                                             # line length beyond DEPTH (m); negative: a taut mooring, pretensioned
PER_CLASS = 512


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=64, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    c1 = scenes.scene_c1()
    n = PER_CLASS * len(STIFFNESS) * len(SLACK)
    pr = np.tile(c1.params[:1].astype(np.float32), (n, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(n)
    st = np.zeros((n, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2] = 37.0 * (i % 72), 41.0 * (i // 72), z_eq
    yaw = 2.0 * np.pi * (i % 64) / 64.0
    st[:, 5], st[:, 6] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
    dt = float(np.float32(1.0 / 60.0))
    sc = scenes.Scene("design loads", st, np.zeros((n, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    cls = i % (len(STIFFNESS) * len(SLACK))                           # the classes interleaved over the field
    k0, c0 = Mooring.for_body(mass, dt)
    k = k0 * np.asarray(STIFFNESS)[cls // len(SLACK)]
    length = DEPTH + np.asarray(SLACK)[cls % len(SLACK)]
    anchors = np.stack([st[:, 0], st[:, 1], np.full(n, z_eq - DEPTH)], axis=1).astype(np.float64)

    sea = SeaState.regular(0.4, 8.0, 0.0, g=sc.g, current=(0.5, 0.0, 0.0))
    omega = 2.0 * np.pi / 5.0                                         # a second, shorter train across the first: 0.2 m, 5 s, from 60 degrees
    kappa = omega * omega / sc.g
    sea.add_wave(0.1, kappa * np.cos(np.pi / 3), kappa * np.sin(np.pi / 3), omega, 1.0)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    sim.set_mooring(anchors, length=length, stiffness=k, damping=c0)
    extremes = sim.track_extremes()                                   # seeded from the state of release
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    rec = extremes.bodies()
    peak, circle = extremes.tension_max(), extremes.excursion(anchors[:, 0:2])
    sim.close()

    print(f"{n} buoys, {args.steps} steps ({args.steps * dt:.1f} s) in one resident run; per design class, the worst of {PER_CLASS} buoys")
    print("  stiffness N/m   line m   peak tension N   watch circle m   lowest z m   top speed m/s")
    for j in range(len(STIFFNESS) * len(SLACK)):
        m = cls == j
        print(f"  {k[m][0]:13.0f}   {length[m][0]:6.2f}   peak tension {peak[m].max():8.1f} N   {circle[m].max():14.3f}   "
              f"{rec[m, 4].min():+10.3f}   {np.sqrt(rec[m, 6].max()):13.3f}")
    if not (peak > 0.0).any():
        raise SystemExit("no line ever carried load")
    if not np.isfinite(rec).all():
        raise SystemExit("a buoy's record is not finite")
    return {"record": rec, "class": cls}


if __name__ == "__main__":
    main()
