#!/usr/bin/env python3
"""Design loads of a spread mooring in an IRREGULAR sea: 1 152 copies of config 1's buoy (a floating unit cube, 500 kg), each on
three lines at 120 degrees to anchors 20 m down, in a JONSWAP sea of significant wave height 1.5 m and peak period 7 s with cos^2
spreading, on a 0.4 m/s current.  The copies differ in what a designer varies - the lines' stiffness (three values) and their
pretension (three values), nine designs - and in where they float, so each meets the sea at a phase of its own.  ONE resident
run carries all of them through the storm (`ClosedLoopSim.set_sea` with a `sea.SeaSpectrum`: 64 wave components evaluated inside
every step of the kernel); `track_extremes()` keeps each buoy's peak line tension and the box it stayed in.

One buoy is watched by the trajectory recorder, and the run checks itself on it: at the recorded positions the surface elevation
the DEVICE used (`HydroEngine.sea_spectrum_sample`) must be `SeaSpectrum.elevation`, the host's fp64 sum, to 1e-4 m.

    python examples/irregular_sea_design_loads.py --steps 3600
"""
import argparse
import os
import sys

import numpy as np
import torch

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
WATCHED = 5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=64, help="physics steps per kernel launch")
    ap.add_argument("--seed", type=int, default=0, help="the seed of the sea's phases and headings")
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
    sc = scenes.Scene("irregular sea design loads", st, np.zeros((n, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    centre = st[:, 0:2].astype(np.float64)
    design = i % designs                                              # the designs interleaved over the field
    k0, c0 = MooringSpread.for_body(mass, dt, LINES)
    k = np.repeat((k0 * np.asarray(STIFFNESS)[design // len(PRETENSION)])[:, None], LINES, axis=1)
    reach = float(np.hypot(RADIUS, DEPTH + z_eq))
    length = np.repeat((reach - np.asarray(PRETENSION)[design % len(PRETENSION)])[:, None], LINES, axis=1)
    lines = MooringSpread.radial(LINES, RADIUS, DEPTH, centre=centre, length=length, stiffness=k, damping=c0)
    anchors = lines.anchors

    sea = jonswap(HS, TP, HEADING, spread="cos2", seed=args.seed, current=(0.4, 0.0, 0.0), g=sc.g)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    sim.set_mooring_spread(anchors, length=length, stiffness=k, damping=c0)
    extremes = sim.track_extremes()                                   # seeded from the state of release
    rec = sim.record([WATCHED], every=1, rows=args.steps)
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    peak, excursion = extremes.tension_max(), extremes.excursion(centre)
    box = extremes.bodies()
    track, steps = rec.states()[:, 0, :], rec.steps()

    # the self-check: the device's surface at the watched buoy's recorded positions against the host's fp64 sum
    rows = np.unique(np.linspace(0, len(steps) - 1, 8).astype(int))
    worst = 0.0
    for r in rows:
        probe = torch.from_numpy(scenes.to_tiled(np.repeat(track[r:r + 1], 64, axis=0))).to(sim.engine.device)
        water = scenes.from_tiled(sim.engine.sea_spectrum_sample(probe, 64, int(steps[r]), dt).cpu().numpy(), 64)
        worst = max(worst, abs(float(water[0, 0]) - float(sea.elevation(track[r, 0], track[r, 1], steps[r] * dt))))
    eta = sea.elevation(track[:, 0], track[:, 1], steps * dt)
    follows = float(np.sqrt(np.mean((track[:, 2] - z_eq - eta) ** 2)))
    sim.close()

    print(f"{n} buoys on {LINES} lines each, {args.steps} steps ({args.steps * dt:.1f} s) in one resident run; JONSWAP Hs {HS} m, Tp {TP} s, "
          f"{len(sea.waves)} components (hs() = {sea.hs():.3f} m); per design, the worst of {PER_DESIGN} buoys")
    print("  stiffness N/m   pretension m   peak tension N   excursion m   lowest z m   highest z m")
    for j in range(designs):
        m = design == j
        print(f"  {k[m][0, 0]:13.0f}   {PRETENSION[j % len(PRETENSION)]:12.2f}   peak tension {peak[m].max():8.1f} N   {excursion[m].max():11.3f}   "
              f"{box[m, 4].min():+10.3f}   {box[m, 5].max():+11.3f}")
    print(f"watched buoy {WATCHED}: rms of z - z_eq - eta over the run {follows:.3f} m (rms eta {float(np.sqrt(np.mean(eta ** 2))):.3f} m)")
    print(f"surface check at {len(rows)} recorded positions: largest |device eta - SeaSpectrum.elevation| = {worst:.2e} m")
    if not worst <= 1e-4:
        raise SystemExit("the device's surface is not the host's")
    if not (peak > 0.0).any():
        raise SystemExit("no line ever carried load")
    if not np.isfinite(box).all():
        raise SystemExit("a buoy's record is not finite")
    return {"tension_max": peak, "excursion": excursion, "design": design, "surface_error": worst}


if __name__ == "__main__":
    main()
