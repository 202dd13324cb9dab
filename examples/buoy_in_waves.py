#!/usr/bin/env python3
"""A moored buoy in moving water: config 1's buoy (a floating unit cube, 500 kg) in a regular deep-water wave of 0.4 m height
and 8 s period travelling along +x, on a 0.3 m/s current, held against the drift by a horizontal-only pose hold - a soft
spring and damper in x and y, nothing in z: its mooring.  The sea state lives inside the stepping kernel
(`ClosedLoopSim.set_sea`): the wave phase advances with every physics step while the body stays resident in registers, and a
trajectory recorder writes every step from inside the launches.  The log becomes the reference's `velocity_log.csv`; the
script prints how closely the buoy follows the surface, max |z - z_eq - eta| with eta the elevation at the buoy's recorded
position and time.

    python examples/buoy_in_waves.py --steps 9600 --chunk 960 --out /tmp/demo
"""
import argparse
import datetime
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.sea import SeaState                         # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402
from silver2_isaacsim_amd.telemetry import write_velocity_log         # noqa: E402

MOORING_N_PER_M, MOORING_N_S_PER_M = 20.0, 40.0                       # surge period ~31 s: well off the 8 s wave


def main(argv=None, steps=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9600)
    ap.add_argument("--chunk", type=int, default=960, help="physics steps per kernel launch")
    ap.add_argument("--out", default=".")
    args = ap.parse_args(argv)
    if steps is not None:
        args.steps = steps
    os.makedirs(args.out, exist_ok=True)

    sc = scenes.scene_c1()
    sea = SeaState.regular(0.4, 8.0, 0.0, g=sc.g, current=(0.3, 0.0, 0.0))
    z_eq = 0.5 * float(sc.params[0, 2]) - float(sc.params[0, 10]) / (sc.rho * float(sc.params[0, 0] * sc.params[0, 1]))
    sc.state[0, 2] = z_eq + sea.elevation(0.0, 0.0, 0.0)              # released at rest at its draught on the surface of t = 0
    sc.state[0, 7:10] = 0.0
    sim = ClosedLoopSim(sc)
    sim.set_sea(sea)
    sim.set_pose_hold(position=sc.state[:, 0:3], kp_lin=(MOORING_N_PER_M, MOORING_N_PER_M, 0.0),
                      kd_lin=(MOORING_N_S_PER_M, MOORING_N_S_PER_M, 0.0))
    rec = sim.record([0], every=1, rows=args.steps)
    sim.run_resident(args.steps, chunk=args.chunk)
    path = write_velocity_log(args.out, rec, 0, start=datetime.datetime.now(), dt=sim.dt)
    s = rec.states()[:, 0].astype(np.float64)
    t = rec.steps() * sim.dt
    deviation = np.abs(s[:, 2] - z_eq - sea.elevation(s[:, 0], s[:, 1], t))
    print(f"{len(s)} rows -> {path}")
    print(f"buoy x: {s[:, 0].min():+.3f} .. {s[:, 0].max():+.3f} m on its mooring (current {sea.current[0]:.1f} m/s), "
          f"z: {s[:, 2].min():+.3f} .. {s[:, 2].max():+.3f} m (wave amplitude {sea.waves[0][0]:.1f} m, z_eq {z_eq:+.4f} m)")
    print(f"largest |z - z_eq - eta| over {len(s)} steps ({t[-1]:.1f} s): {deviation.max():.4f} m")
    sim.close()
    return {"csv": path, "rows": len(s), "deviation": float(deviation.max()), "states": s}


if __name__ == "__main__":
    main()
