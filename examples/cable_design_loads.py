#!/usr/bin/env python3
"""The design loads of an umbilical, read off ONE resident run: the cable of examples/umbilical_cable.py - config 1's buoy moored
on a seabed 40 m down in a 0.2 m/s current, an ROV below it on a string of eight small boxes joined by nine links of 1.5 m - in
SIX designs side by side, one tile of 64 bodies each: three cable weights (boxes of 28.5, 30 and 31.5 kg; each displaces 27.7 kg
of water) times two ROVs (140 and 160 kg).  What sizes such a cable is the largest tension each link ever carried.
`ClosedLoopSim.track_link_tensions()` keeps that maximum inside the stepping kernel, per link, in every physics step
(hydro_step_fused_tiled_multi_peak): no trajectory is recorded, nothing is read back between the launches, and the table below
is one small copy at the end - the way examples/mooring_design_loads.py reads the design loads of its mooring lines off the
extremes record.  (A design's peak can lie a little below its tension at the end while the cable is still settling: the record
samples the state each step starts from, and the final state starts no step.)  The script prints the peak
tension of every link of every design beside the link's tension at the end and the submerged weight hanging below it, and checks
itself: every link carried load, for either ROV a heavier cable loads its top link more, and the record's two ends of every
link agree bit for bit.

    python examples/cable_design_loads.py --steps 3600 --chunk 600
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
SEGMENTS, SEGMENT_SIDE = 8, 0.3
ROV_BOX = (0.6, 0.5, 0.4)                                             # 123 kg of water displaced
DESIGNS = [(segment, rov) for rov in (140.0, 160.0) for segment in (28.5, 30.0, 31.5)]      # (mass of a cable box, mass of the ROV), kg
BODIES = SEGMENTS + 2                                                 # of one design: buoy, boxes, ROV
SPACING = 30.0                                                        # m between the designs, across the current


def scene():
    """One tile of 64 per design: lanes 0 .. 9 the buoy at rest at its draught, the cable's boxes and the ROV in a line straight
    below it, every link slack by a twentieth; lanes 10 .. 63 spare buoys at rest, 30 m further downstream each, tied to nothing."""
    c1 = scenes.scene_c1()
    n = 64 * len(DESIGNS)
    pr = np.tile(c1.params[:1], (n, 1)).astype(np.float32)
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    st = np.zeros((n, 13), np.float32)
    st[:, 6] = 1.0
    st[:, 2] = z_eq
    for d, (segment, rov) in enumerate(DESIGNS):
        b = 64 * d
        st[b:b + 64, 1] = SPACING * d
        st[b + BODIES:b + 64, 0] = SPACING * np.arange(1, 64 - BODIES + 1)
        pr[b + 1:b + BODIES - 1, 0:3], pr[b + 1:b + BODIES - 1, 10] = SEGMENT_SIDE, segment
        pr[b + BODIES - 1, 0:3], pr[b + BODIES - 1, 10] = ROV_BOX, rov
        # the schema's linear and angular damping are absolute constants (for the unit cube): the smaller bodies take them in
        # proportion to their face area and to its square
        area = pr[b + 1:b + BODIES, 0] * pr[b + 1:b + BODIES, 1]
        pr[b + 1:b + BODIES, 5], pr[b + 1:b + BODIES, 6] = pr[0, 5] * area, pr[0, 6] * area ** 2
        st[b + 1:b + BODIES, 2] = z_eq - 0.5 - 0.95 * LINK * np.arange(1, BODIES)
    return scenes.Scene("cable design loads", st, np.zeros((n, 6), np.float32), pr, dt=c1.dt, rho=c1.rho, g=c1.g)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=600, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    sc = scene()
    mass = sc.params[:, 10].astype(np.float64)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(SeaState((CURRENT, 0.0, 0.0)))
    sim.set_seabed(Seabed.for_step(-DEPTH, sim.dt))
    buoys = 64 * np.arange(len(DESIGNS))
    mk, mc = Mooring.for_body(mass[buoys], sim.dt)
    anchors = np.stack([np.zeros(len(DESIGNS)), SPACING * np.arange(len(DESIGNS)), np.full(len(DESIGNS), -DEPTH)], axis=1)
    sim.set_mooring(anchors, fairlead=(0.0, 0.0, -0.5), length=MOORING, stiffness=mk, damping=mc, bodies=buoys)
    # per design: the chain's uniform constants, the damper at for_chain's default, the spring at half the per-body stability bound
    links, fair_a, stiffness, damping = [], [], [], []
    for b in buoys:
        chain = b + np.arange(BODIES)
        k, c = TetherNet.for_chain(mass[chain], sim.dt)
        links.append(np.stack([chain[:-1], chain[1:]], axis=1))
        fair_a.append([(0.0, 0.0, -0.5)] + [(0.0, 0.0, 0.0)] * (BODIES - 2))       # the buoy's underside, then centre to centre
        stiffness += [k * 0.5 * STABLE / DEFAULT_K] * (BODIES - 1)
        damping += [c] * (BODIES - 1)
    per_design = BODIES - 1
    net = dict(links=np.concatenate(links), fairlead_a=np.concatenate(fair_a), length=LINK, stiffness=np.array(stiffness), damping=np.array(damping),
               layer=np.tile(np.arange(per_design) % 2, len(DESIGNS)))
    sim.set_tether_net(**net)
    assert sim.tether_layers == 2
    loads = sim.track_link_tensions()
    sim.run_resident(args.steps, chunk=min(args.chunk, args.steps))
    record = loads.record()                                           # (n, 2): one small copy, no trajectory
    peak = loads.peak(record).astype(np.float64).reshape(len(DESIGNS), per_design)
    other_end = record[net["links"][:, 1], net["layer"]].astype(np.float64).reshape(peak.shape)
    last = sim.state().astype(np.float64)
    sim.close()
    at_end = TetherNet(n=sc.n, **net).tensions(last).reshape(peak.shape)
    volume = np.prod(sc.params[:, 0:3].astype(np.float64), axis=1)
    weight = (mass - sc.rho * volume) * sc.g
    print(f"{args.steps} steps ({args.steps * sim.dt:.1f} s) in a {CURRENT} m/s current, {len(DESIGNS)} designs of a cable of {SEGMENTS} boxes and "
          f"{per_design} links of {LINK} m, one tile each, {sim.tether_layers} layers; link 0 is the buoy's, link {per_design - 1} the ROV's")
    for d, (segment, rov) in enumerate(DESIGNS):
        below = np.cumsum(weight[64 * d + 1:64 * d + BODIES][::-1])[::-1]
        print(f"design {d}: boxes of {segment:g} kg, ROV of {rov:g} kg, k {stiffness[per_design * d]:.0f} N/m")
        print("  peak tension per link (N):        " + " ".join(f"{t:7.1f}" for t in peak[d]))
        print("  tension at the end (N):           " + " ".join(f"{t:7.1f}" for t in at_end[d]))
        print("  submerged weight below (N):       " + " ".join(f"{w:7.1f}" for w in below))
    print(f"largest peak tension of any link: {peak.max():.1f} N (design {int(peak.max(axis=1).argmax())}, link {int(peak.max(axis=0).argmax())})")
    if not (peak > 0.0).all():
        raise SystemExit("a link never carried load")
    top = peak[:, 0].reshape(2, 3)                                    # (per ROV, the cables in ascending weight)
    if not (np.diff(top, axis=1) > 0.0).all():
        raise SystemExit("a heavier cable did not load its top link more")
    if not np.array_equal(peak, other_end):
        raise SystemExit("the two ends of a link disagree")
    untied = np.ones(sc.n, bool)
    untied[net["links"].reshape(-1)] = False
    if record[untied].any():
        raise SystemExit("a body without a line has a tension on record")
    return {"peak": peak, "at_end": at_end}


if __name__ == "__main__":
    main()
