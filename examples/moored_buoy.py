#!/usr/bin/env python3
"""A buoy on a mooring line: config 1's buoy (a floating unit cube, 500 kg) anchored on a seabed 20 m down by one tension-only
line (`ClosedLoopSim.set_mooring`), in a 0.5 m/s current and a regular deep-water wave of 0.4 m height and 8 s period along +x.
Sea, bed and line all live inside the stepping kernel: the line's spring and damper are evaluated in every physics step from
the state that step starts from, while the body stays resident in registers, and a trajectory recorder writes every step
from inside the launches.  Without the line the buoy leaves the scene with the current; with it, it rides the waves on
station.  The script checks itself: the buoy stays within the line's reach and the line carries load.

    python examples/moored_buoy.py --steps 3600 --chunk 600
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
from silver2_isaacsim_amd.seabed import Seabed                        # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

DEPTH, LINE = 20.0, 19.6                                              # the bed below the still surface and the line's length (m)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=600, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    sc = scenes.scene_c1()
    mass = float(sc.params[0, 10])
    z_eq = 0.5 * float(sc.params[0, 2]) - mass / (sc.rho * float(sc.params[0, 0] * sc.params[0, 1]))
    sea = SeaState.regular(0.4, 8.0, 0.0, g=sc.g, current=(0.5, 0.0, 0.0))
    sc.state[0, 2] = z_eq + sea.elevation(0.0, 0.0, 0.0)              # released at rest at its draught on the surface of t = 0
    sc.state[0, 7:10] = 0.0
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    sim.set_seabed(Seabed.for_step(-DEPTH, sim.dt))
    k, c = Mooring.for_body(mass, sim.dt)                             # the stable defaults for this mass and step
    anchor = (0.0, 0.0, -DEPTH)                                       # on the bed, under the point of release
    sim.set_mooring(anchor, fairlead=(0.0, 0.0, -0.5), length=LINE, stiffness=k, damping=c)
    rec = sim.record([0], every=1, rows=args.steps)
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    s = rec.states()[:, 0].astype(np.float64)
    line = Mooring(anchor, fairlead=(0.0, 0.0, -0.5), length=LINE, stiffness=k, damping=c)
    tension = np.array([line.tension(row[None, :])[0] for row in s])
    reach = np.array([line.geometry(row[None, :])[2][0] for row in s])
    sim.close()
    print(f"{len(s)} steps ({len(s) * sim.dt:.1f} s): buoy x {s[:, 0].min():+.3f} .. {s[:, 0].max():+.3f} m, z {s[:, 2].min():+.3f} .. {s[:, 2].max():+.3f} m "
          f"(current {sea.current[0]:.1f} m/s, wave amplitude {sea.waves[0][0]:.1f} m)")
    print(f"fairlead to anchor: at most {reach.max():.3f} m of {LINE} m of line; taut in {np.mean(tension > 0) * 100:.0f} % of the steps")
    print(f"mean tension {tension.mean():.1f} N (largest {tension.max():.1f} N; k = {k:.0f} N/m, c = {c:.0f} N s/m)")
    if not reach.max() < 1.02 * LINE:
        raise SystemExit("the buoy left the line's reach")
    if not tension.max() > 0.0:
        raise SystemExit("the line never carried load")
    return {"states": s, "tension": tension}


if __name__ == "__main__":
    main()
