#!/usr/bin/env python3
"""Design loads in DEEP and in SHALLOW water, side by side: the 1 152 buoys of examples/irregular_sea_design_loads.py (config 1's
buoy on three lines at 120 degrees to anchors 20 m down, nine designs of stiffness and pretension, 128 buoys each) in the same
JONSWAP sea of Hs 1.5 m and Tp 7 s with cos^2 spreading on a 0.4 m/s current - the same bins, amplitudes, phases and headings -
once over infinitely deep water and once over h = 20 m, where the anchors are (`jonswap(..., depth=20.0)`: every component's
wavenumber from omega^2 = g kappa tanh(kappa h), and `ClosedLoopSim.set_sea` steps it through hydro_step_fused_tiled_multi_fd).
At Tp = 7 s, kappa h is about 1.7 there: the wave is shorter, its horizontal orbital velocity at the surface larger by
coth(kappa h), and it reaches the bed.

Per design the run prints the peak line tension (the median buoy's `tension_max`) and the standard deviation of the tension from
the response statistics, deep beside shallow.

    python examples/shallow_water_design_loads.py --steps 3600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import MooringSpread                # noqa: E402
from silver2_isaacsim_amd.sea import jonswap, wavenumber              # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

LINES, RADIUS, DEPTH = 3, 15.0, 20.0                                  # the anchors: on a circle of 15 m, 20 m below the surface - on the bed
STIFFNESS = (0.5, 1.0, 2.0)                                           # times MooringSpread.for_body's default
PRETENSION = (0.0, 0.1, 0.3)                                          # each line this much shorter than its reach at rest (m)
PER_DESIGN = 128
HS, TP, HEADING = 1.5, 7.0, 25.0


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
    sc = scenes.Scene("shallow water design loads", st, np.zeros((n, 6), np.float32), pr, dt=dt, rho=c1.rho, g=c1.g)
    centre = st[:, 0:2].astype(np.float64)
    design = i % designs                                              # the designs interleaved over the field
    k0, c0 = MooringSpread.for_body(mass, dt, LINES)
    k = np.repeat((k0 * np.asarray(STIFFNESS)[design // len(PRETENSION)])[:, None], LINES, axis=1)
    reach = float(np.hypot(RADIUS, DEPTH + z_eq))
    length = np.repeat((reach - np.asarray(PRETENSION)[design % len(PRETENSION)])[:, None], LINES, axis=1)
    anchors = MooringSpread.radial(LINES, RADIUS, DEPTH, centre=centre, length=length, stiffness=k, damping=c0).anchors

    results = {}
    for name, depth in (("deep", None), ("shallow", DEPTH)):
        sea = jonswap(HS, TP, HEADING, spread="cos2", seed=args.seed, current=(0.4, 0.0, 0.0), g=sc.g, depth=depth)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.set_sea(sea)
        sim.set_mooring_spread(anchors, length=length, stiffness=k, damping=c0)
        extremes = sim.track_extremes()
        stat = sim.track_statistics(("z", "tension"))
        sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
        if not (stat.count() == args.steps).all():
            raise SystemExit("the record has not counted every step")
        results[name] = dict(peak=extremes.tension_max(), sigma=stat.std("tension"), box=extremes.bodies())
        sim.close()
        if not (np.isfinite(results[name]["box"]).all() and np.isfinite(results[name]["sigma"]).all() and (results[name]["peak"] > 0.0).any()):
            raise SystemExit("a buoy's record is not finite, or no line ever carried load")

    omega_p = 2.0 * np.pi / TP
    kh = wavenumber(omega_p, DEPTH, sc.g) * DEPTH
    print(f"{n} buoys on {LINES} lines each, {args.steps} steps ({args.steps * dt:.1f} s) per resident run; JONSWAP Hs {HS} m, Tp {TP} s, 64 components; "
          f"deep water beside h = {DEPTH:g} m (kappa_p h = {kh:.2f}, peak wavelength {2.0 * np.pi * sc.g / omega_p ** 2:.0f} m -> "
          f"{2.0 * np.pi * DEPTH / kh:.0f} m, surface velocity x {1.0 / np.tanh(kh):.2f}); per design the median buoy")
    for j in range(designs):
        m = design == j
        peak = [float(np.median(results[w]["peak"][m])) for w in ("deep", "shallow")]
        sigma = [float(np.median(results[w]["sigma"][m])) for w in ("deep", "shallow")]
        print(f"  stiffness {k[m][0, 0]:7.0f} N/m  pretension {PRETENSION[j % len(PRETENSION)]:4.2f} m:  peak tension {peak[0]:8.1f} N deep {peak[1]:8.1f} N at h = {DEPTH:g} m "
              f"({100.0 * (peak[1] / max(peak[0], 1e-30) - 1.0):+5.1f} %)   sigma {sigma[0]:7.1f} N deep {sigma[1]:7.1f} N at h = {DEPTH:g} m")
    return {"design": design, **{f"{w}_{q}": results[w][q] for w in results for q in ("peak", "sigma")}}


if __name__ == "__main__":
    main()
