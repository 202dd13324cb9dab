#!/usr/bin/env python3
"""The buoy of plugin_buoy_in_waves.py in an IRREGULAR sea through the plugin surface: config 1's buoy (a floating unit cube,
500 kg) carries a `HydrodynamicsBehavior` on the in-memory simulator host; the host integrates (a semi-implicit Euler point mass
stands in for PhysX) and the plugin supplies the wrench, one fused launch per physics step.  `HydrodynamicsBehavior.set_sea`
takes a JONSWAP sea of 64 components (Hs 0.6 m, Tp 6 s, cos^2 spreading) on a 0.3 m/s current - with `--depth` the same sea
over a bottom that many metres down, built with the dispersion relation of that depth.  The plugin evaluates it at its own clock,
the sum of the physics steps' delta times.  Nothing moors the buoy.  The script prints the drift, how closely the buoy follows
the surface - max |z - z_eq - eta| against the significant wave height - and the standard deviation of its heave against the
sea's own, Hs / 4.

    python examples/plugin_buoy_in_irregular_sea.py --steps 1800
    python examples/plugin_buoy_in_irregular_sea.py --steps 1800 --depth 8
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import behavior as hb                      # noqa: E402
from silver2_isaacsim_amd import config as cfg                       # noqa: E402
from silver2_isaacsim_amd import scenes                              # noqa: E402
from silver2_isaacsim_amd.sea import jonswap                         # noqa: E402
from silver2_isaacsim_amd.testing import FakeHost, FakeWorld         # noqa: E402

BUOY = "/World/Environment/Buoy"
ATTRS = ("xDimension", "yDimension", "zDimension", "linearDragCoefficient", "angularDragCoefficient", "linearDamping",
         "angularDamping", "liftCoefficient", "linearAddedMassCoefficient", "angularAddedMassCoefficient")      # the engine's parameter order


def main(argv=None, steps=None, depth=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1800)
    ap.add_argument("--depth", type=float, default=None, help="still-water depth in m (default: deep water)")
    args = ap.parse_args(argv)
    if steps is not None:
        args.steps = steps
    if depth is not None:
        args.depth = depth

    sc = scenes.scene_c1()
    dt, mass = sc.dt, float(sc.params[0, 10])
    sea = jonswap(0.6, 6.0, 0.0, seed=7, spread="cos2", current=(0.3, 0.0, 0.0), g=sc.g, depth=args.depth)
    z_eq = 0.5 * float(sc.params[0, 2]) - mass / (sc.rho * float(sc.params[0, 0] * sc.params[0, 1]))
    hb.REGISTRY.clear()
    world = FakeWorld("cuda:0")
    host = FakeHost(world)
    prim = cfg.AttributeStore("Buoy", BUOY)
    # released at rest at its draught on the surface of t = 0
    world.add_body(BUOY, (0.0, 0.0, z_eq + float(sea.elevation(0.0, 0.0, 0.0))), (1.0, 0.0, 0.0, 0.0), [0.0] * 6, mass)
    b = hb.HydrodynamicsBehavior(prim, host)
    b.on_init()
    for name, value in zip(ATTRS, sc.params[0, :10]):
        host.set_exposed_variable(prim, cfg.full_attr_name(name), float(value))
    b.set_sea(sea)                                                # scene-wide; a SeaSpectrum, with a depth a finite-depth sea
    b.on_play()                                                   # the clock of the buoy's stepping unit starts here

    track = np.empty((args.steps, 4))                             # t, x, y, z AFTER each step
    for k in range(args.steps):
        host.step(dt)                                             # the plugin's callback: the wrench at time b.sea_time
        world.integrate([BUOY], dt, sc.g)                         # "PhysX"
        track[k] = (b.sea_time, *world.positions[0].tolist())
    v = world.velocities[0, 0:3].tolist()
    b.on_stop()
    hb.REGISTRY.clear()
    t, x, y, z = track.T
    eta = np.array([float(sea.elevation(xi, yi, ti)) for xi, yi, ti in zip(x, y, t)])
    deviation = np.abs(z - z_eq - eta)
    water = "deep water" if args.depth is None else f"h = {args.depth:g} m"
    print(f"{args.steps} physics steps of {dt:.5f} s through HydrodynamicsBehavior, {world.apply_calls} wrenches applied; "
          f"JONSWAP Hs {sea.hs():.2f} m, Tp 6 s, {len(sea.waves)} components, {water}")
    print(f"drift: x {x[-1]:+.3f} m, y {y[-1]:+.3f} m after {t[-1]:.1f} s; final velocity ({v[0]:+.3f}, {v[1]:+.3f}) m/s "
          f"in a current of ({sea.current[0]:.1f}, {sea.current[1]:.1f}) m/s")
    print(f"heave: z - z_eq {(z - z_eq).min():+.3f} .. {(z - z_eq).max():+.3f} m, sigma {np.std(z - z_eq):.3f} m (the sea's: Hs / 4 = {sea.hs() / 4:.3f} m)")
    print(f"largest |z - z_eq - eta| over {args.steps} steps ({t[-1]:.1f} s): {deviation.max():.4f} m")
    return {"track": track, "deviation": float(deviation.max()), "velocity": v, "apply_calls": world.apply_calls, "eta": eta}


if __name__ == "__main__":
    main()
