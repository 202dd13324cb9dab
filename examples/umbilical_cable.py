#!/usr/bin/env python3
"""A lumped-mass umbilical: config 1's buoy (a floating unit cube, 500 kg), moored on a seabed 40 m down in a 0.2 m/s current,
carries an ROV on a CABLE - not one massless spring, but a string of eight small boxes (0.3 m cubes of 28.5 kg, 27.7 kg of water
displaced each) joined by nine links of 1.5 m (`ClosedLoopSim.set_tether_net`, `TetherNet.chain`).  Every cable body is an
ordinary body of the scene: it has mass, buoyancy and drag from the hydrodynamics every body has, so the cable SAGS under its
own submerged weight and BOWS downstream in the current, and its tension grows from the ROV up to the buoy - three things the
single line of examples/tethered_rov.py cannot show.  A chain costs two layers of tether records (links 0, 2, 4, ... in layer
0, links 1, 3, 5, ... in layer 1); all ten bodies lie in one tile of 64, each link's two ends exchange their fairleads between
lanes inside the stepping kernel, and the scene runs resident, many steps per launch.  The script prints the cable's shape and
the link tensions and checks itself: the links carry load, the top link carries more than the bottom one, and no link is
stretched past half its length (the springs are explicit, so a light cable body bounds their stiffness: `TetherNet.for_chain`).

    python examples/umbilical_cable.py --steps 3600 --chunk 600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.mooring import DEFAULT_K, Mooring, STABLE   # noqa: E402
from silver2_isaacsim_amd.sea import SeaState                         # noqa: E402
from silver2_isaacsim_amd.seabed import Seabed                        # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402
from silver2_isaacsim_amd.tether import TetherNet                     # noqa: E402

CURRENT = 0.2                                                         # m/s, along x
DEPTH, MOORING, LINK = 40.0, 39.6, 1.5                                # the bed below the still surface; the mooring line's and each link's length (m)
SEGMENTS, SEGMENT_SIDE, SEGMENT_MASS = 8, 0.3, 28.5
ROV_BOX, ROV_MASS = (0.6, 0.5, 0.4), 126.0                         # 123 kg of water displaced


def scene():
    """Ten bodies in one tile: 0 the buoy at rest at its draught, 1 .. 8 the cable's boxes and 9 the ROV, at rest in a line
    straight below it, every link slack by a twentieth."""
    c1 = scenes.scene_c1()
    n = SEGMENTS + 2
    pr = np.tile(c1.params[:1], (n, 1)).astype(np.float32)
    pr[1:-1, 0:3], pr[1:-1, 10] = SEGMENT_SIDE, SEGMENT_MASS
    pr[-1, 0:3], pr[-1, 10] = ROV_BOX, ROV_MASS
    # the schema's linear and angular damping are absolute constants (300 N s/m, 150 N m s for the unit cube): the smaller
    # bodies take them in proportion to their face area and to its square
    area = pr[1:, 0] * pr[1:, 1]
    pr[1:, 5], pr[1:, 6] = pr[0, 5] * area, pr[0, 6] * area ** 2
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    st = np.zeros((n, 13), np.float32)
    st[:, 6] = 1.0
    st[:, 2] = z_eq - 0.5 - 0.95 * LINK * np.arange(n)
    st[0, 2] = z_eq
    return scenes.Scene("umbilical cable", st, np.zeros((n, 6), np.float32), pr, dt=c1.dt, rho=c1.rho, g=c1.g)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=600, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    sc = scene()
    n = sc.n
    mass = sc.params[:, 10].astype(np.float64)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(SeaState((CURRENT, 0.0, 0.0)))
    sim.set_seabed(Seabed.for_step(-DEPTH, sim.dt))
    mk, mc = Mooring.for_body(mass[0], sim.dt)
    anchor = (0.0, 0.0, -DEPTH)
    sim.set_mooring(anchor, fairlead=(0.0, 0.0, -0.5), length=MOORING, stiffness=mk, damping=mc, bodies=[0])
    # uniform constants for the chain: the damper at for_chain's default, the spring at half the per-body stability bound
    k, c = TetherNet.for_chain(mass, sim.dt)
    k *= 0.5 * STABLE / DEFAULT_K
    cable = dict(length=LINK, stiffness=k, damping=c)
    # the buoy's underside, then centre to centre along the cable
    links = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    fair_a = np.zeros((n - 1, 3))
    fair_a[0] = (0.0, 0.0, -0.5)
    net = dict(links=links, fairlead_a=fair_a, layer=np.arange(n - 1) % 2, **cable)                # (what TetherNet.chain builds, with the buoy's own fairlead)
    sim.set_tether_net(**net)
    assert sim.tether_layers == 2
    rec = sim.record(list(range(n)), every=1, rows=args.steps)
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    s = rec.states().astype(np.float64)                               # (steps, n, 13)
    sim.close()
    lines = TetherNet(n=n, **net)
    tension = np.array([lines.tensions(row) for row in s])            # (steps, n - 1)
    last = s[-1]
    p = last[:, 0:3].copy()
    p[0, 2] -= 0.5                                                     # the buoy's fairlead
    length = np.linalg.norm(np.diff(p, axis=0), axis=1)
    # sag and bow: how far the cable's bodies leave the straight line from the buoy's fairlead to the ROV
    chord = p[-1] - p[0]
    along = np.clip((p - p[0]) @ chord / (chord @ chord), 0.0, 1.0)
    off = p - (p[0] + along[:, None] * chord)
    mid = int(np.argmax(np.linalg.norm(off, axis=1)))
    weight = (mass[1:] - sc.rho * np.prod(sc.params[1:, 0:3].astype(np.float64), axis=1)) * sc.g
    print(f"{len(s)} steps ({len(s) * sim.dt:.1f} s) in a {CURRENT} m/s current: buoy at x {last[0, 0]:+.2f} m, z {last[0, 2]:+.3f} m; "
          f"a cable of {SEGMENTS} boxes and {n - 1} links of {LINK} m, k {k:.0f} N/m, c {c:.2f} N s/m, in {sim.tether_layers} layers")
    print("cable shape (x downstream, z): " + "  ".join(f"({x:+.2f}, {z:+.2f})" for x, z in zip(last[:, 0], last[:, 2])))
    print("link tensions (N): " + " ".join(f"{t:.1f}" for t in tension[-1]))
    print(f"largest link tensions (N): " + " ".join(f"{t:.1f}" for t in tension.max(axis=0)))
    print(f"submerged weight below each link (N): " + " ".join(f"{w:.1f}" for w in np.cumsum(weight[::-1])[::-1]))
    print(f"ROV depth {-last[-1, 2]:.2f} m, {last[-1, 0] - last[0, 0]:+.2f} m downstream of the buoy; the cable leaves the straight line by "
          f"{np.linalg.norm(off[mid]):.2f} m at body {mid}: sag {off[mid, 2]:.2f} m, bow downstream {off[mid, 0]:+.2f} m")
    print(f"links stretched to " + " ".join(f"{x:.2f}" for x in length) + f" m of {LINK} m")
    if not tension.max() > 0.0:
        raise SystemExit("the cable never carried load")
    if not tension[:, 0].max() > tension[:, -1].max():
        raise SystemExit("the top link did not carry more than the bottom one")
    if not length.max() < 1.5 * LINK:
        raise SystemExit("a link is stretched past half its length")
    return {"states": s, "tension": tension}


if __name__ == "__main__":
    main()
