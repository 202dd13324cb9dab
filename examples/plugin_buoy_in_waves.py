#!/usr/bin/env python3
"""A buoy in moving water through the PLUGIN surface: config 1's buoy (a floating unit cube, 500 kg) carries a
`HydrodynamicsBehavior` on the in-memory simulator host, exactly as Kit would instantiate it; the host integrates (a
semi-implicit Euler point mass stands in for PhysX) and the plugin supplies the wrench, one fused launch per physics step.
`HydrodynamicsBehavior.set_sea` puts a 0.3 m/s current and a regular deep-water wave of 0.4 m height and 8 s period along +x
into the scene; the plugin evaluates them at its own clock, the sum of the physics steps' delta times.  Nothing moors the
buoy: it is carried off by the current while it rides the wave.  The script prints the drift and how closely the buoy follows
the surface, max |z - z_eq - eta| with eta the elevation at the buoy's position and time.

    python examples/plugin_buoy_in_waves.py --steps 1800
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
from silver2_isaacsim_amd.sea import SeaState                        # noqa: E402
from silver2_isaacsim_amd.testing import FakeHost, FakeWorld         # noqa: E402

BUOY = "/World/Environment/Buoy"
ATTRS = ("xDimension", "yDimension", "zDimension", "linearDragCoefficient", "angularDragCoefficient", "linearDamping",
         "angularDamping", "liftCoefficient", "linearAddedMassCoefficient", "angularAddedMassCoefficient")      # the engine's parameter order


def main(argv=None, steps=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1800)
    args = ap.parse_args(argv)
    if steps is not None:
        args.steps = steps

    sc = scenes.scene_c1()
    dt, mass = sc.dt, float(sc.params[0, 10])
    sea = SeaState.regular(0.4, 8.0, 0.0, g=sc.g, current=(0.3, 0.0, 0.0))
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
    b.set_sea(sea)                                                # scene-wide, like the water density and gravity
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
    deviation = np.abs(z - z_eq - sea.elevation(x, y, t))
    print(f"{args.steps} physics steps of {dt:.5f} s through HydrodynamicsBehavior, {world.apply_calls} wrenches applied")
    print(f"drift: x {x[-1]:+.3f} m, y {y[-1]:+.3f} m after {t[-1]:.1f} s; final velocity ({v[0]:+.3f}, {v[1]:+.3f}) m/s "
          f"in a current of ({sea.current[0]:.1f}, {sea.current[1]:.1f}) m/s")
    print(f"z: {z.min():+.3f} .. {z.max():+.3f} m (wave amplitude {sea.waves[0][0]:.1f} m, z_eq {z_eq:+.4f} m)")
    print(f"largest |z - z_eq - eta| over {args.steps} steps ({t[-1]:.1f} s): {deviation.max():.4f} m")
    return {"track": track, "deviation": float(deviation.max()), "velocity": v, "apply_calls": world.apply_calls}


if __name__ == "__main__":
    main()
