#!/usr/bin/env python3
"""An ROV on an umbilical under a moored buoy: config 1's buoy (a floating unit cube, 500 kg) is anchored on a seabed 30 m down
by a mooring line (`ClosedLoopSim.set_mooring`) in a 0.5 m/s current; a slightly heavy ROV (0.6 x 0.5 x 0.4 m, 135 kg against
123 kg of water displaced) hangs from the buoy's underside on 8 m of tether (`ClosedLoopSim.set_tether`).  The tether is the
one force that acts on two bodies at once: inside the stepping kernel each of the two lanes reads the other's fairlead of
the very step from the other's registers, and both get the same tension with opposite signs - so the scene runs resident,
many steps per launch, like every scene of independent bodies.  The current pushes buoy and ROV downstream until the mooring
line holds the buoy and the tether holds the ROV, which trails behind and below it.  The script checks itself: the tether
carries the ROV's submerged weight and more (the current's drag), and the ROV stays within the tether's reach.

    python examples/tethered_rov.py --steps 3600 --chunk 600
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
from silver2_isaacsim_amd.tether import Tether                        # noqa: E402

DEPTH, MOORING, TETHER = 30.0, 29.6, 8.0                              # the bed below the still surface; the two lines' lengths (m)
ROV_BOX, ROV_MASS = (0.6, 0.5, 0.4), 135.0


def scene():
    """(scene of two bodies: 0 the buoy at rest at its draught, 1 the ROV at rest on a slack tether below it; the buoy's draught z)."""
    c1 = scenes.scene_c1()
    pr = np.tile(c1.params[:1], (2, 1)).astype(np.float32)
    pr[1, 0:3], pr[1, 10] = ROV_BOX, ROV_MASS
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    st = np.zeros((2, 13), np.float32)
    st[:, 6] = 1.0
    st[0, 2], st[1, 2] = z_eq, z_eq - 0.5 - 0.95 * TETHER
    return scenes.Scene("tethered rov", st, np.zeros((2, 6), np.float32), pr, dt=c1.dt, rho=c1.rho, g=c1.g), z_eq


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=600, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    sc, z_eq = scene()
    m_buoy, m_rov = float(sc.params[0, 10]), float(sc.params[1, 10])
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(SeaState((0.5, 0.0, 0.0)))
    sim.set_seabed(Seabed.for_step(-DEPTH, sim.dt))
    mk, mc = Mooring.for_body(m_buoy, sim.dt)
    anchor = (0.0, 0.0, -DEPTH)
    sim.set_mooring(anchor, fairlead=(0.0, 0.0, -0.5), length=MOORING, stiffness=mk, damping=mc, bodies=[0])
    tk, tc = Tether.for_pair(m_buoy, m_rov, sim.dt)                   # stable for the pair's reduced mass and this step
    line = dict(pairs=[[0, 1]], fairlead_a=(0.0, 0.0, -0.5), fairlead_b=(0.0, 0.0, 0.2), length=TETHER, stiffness=tk, damping=tc)
    sim.set_tether(**line)
    rec = sim.record([0, 1], every=1, rows=args.steps)
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    s = rec.states().astype(np.float64)                               # (steps, 2, 13)
    sim.close()
    tether = Tether(n=2, **line)
    mooring = Mooring(anchor, fairlead=(0.0, 0.0, -0.5), length=MOORING, stiffness=mk, damping=mc)
    t_teth = np.array([tether.tension(row)[1] for row in s])
    t_moor = np.array([mooring.tension(row[0:1])[0] for row in s])
    reach = np.array([tether.geometry(row)[2][1] for row in s])
    last = s[-1]
    weight = (m_rov - sc.rho * float(np.prod(ROV_BOX))) * sc.g
    print(f"{len(s)} steps ({len(s) * sim.dt:.1f} s) in a 0.5 m/s current: buoy at x {last[0, 0]:+.2f} m, z {last[0, 2]:+.3f} m")
    print(f"ROV depth {-last[1, 2]:.2f} m, downstream {last[1, 0]:.2f} m of the anchor ({last[1, 0] - last[0, 0]:+.2f} m of the buoy)")
    print(f"tether tension {t_teth[-1]:.1f} N (largest {t_teth.max():.1f} N; the ROV's submerged weight {weight:.1f} N), "
          f"taut in {np.mean(t_teth > 0) * 100:.0f} % of the steps; at most {reach.max():.3f} m of {TETHER} m paid out")
    print(f"mooring tension {t_moor[-1]:.1f} N (largest {t_moor.max():.1f} N)")
    if not reach.max() < 1.05 * TETHER:
        raise SystemExit("the ROV left the tether's reach")
    if not t_teth.max() > 0.0:
        raise SystemExit("the tether never carried load")
    return {"states": s, "tether": t_teth, "mooring": t_moor}


if __name__ == "__main__":
    main()
