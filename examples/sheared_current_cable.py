#!/usr/bin/env python3
"""The umbilical of examples/umbilical_cable.py - a moored buoy, a lumped-mass cable of eight boxes, an ROV at its end - under the
SAME SURFACE SPEED twice: once as the uniform current every scene had so far, once as the profile a design code gives
(DNV-RP-C205 4.1: a tidal part that follows a 1/7 power law over the depth, plus a wind-driven slab that dies out linearly over the
top metres, here on another heading).  The buoy at the surface feels the same water in both runs; the cable and the ROV hang
through water that slows down with depth, so under the profile the cable bows less and the ROV is carried less far - a check
against the uniform surface current over-loads everything below the surface, and cannot turn with depth at all
(`ClosedLoopSim.set_current_profile`, `sea.CurrentProfile`; include/hydro.h, "Current profile").  A profile is defined over a water
column, so both runs step through a finite-depth sea without waves (`SeaSpectrum(depth=)`): the uniform current as the sea's own
U, the profile on top of U = 0.  The script prints both shapes and checks itself: the sheared current carries the ROV less far.

    python examples/sheared_current_cable.py --steps 3600 --chunk 600
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from silver2_isaacsim_amd.mooring import DEFAULT_K, Mooring, STABLE   # noqa: E402
from silver2_isaacsim_amd.sea import CurrentProfile, SeaSpectrum      # noqa: E402
from silver2_isaacsim_amd.seabed import Seabed                        # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402
from silver2_isaacsim_amd.tether import TetherNet                     # noqa: E402
from umbilical_cable import DEPTH, LINK, MOORING, scene               # noqa: E402

TIDE, WIND, WIND_HEADING, SLAB = 0.3, 0.3, 30.0, 8.0                  # m/s at the surface, m/s at the surface, degrees, m


def run(sc, sea, profile, steps, chunk):
    """The cable's scene through `sea` (and `profile`): the last state (n, 13) in fp64 and the largest tension of each link (N)."""
    n = sc.n
    mass = sc.params[:, 10].astype(np.float64)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    if profile is not None:
        sim.set_current_profile(profile)
    sim.set_seabed(Seabed.for_step(-DEPTH, sim.dt))
    mk, mc = Mooring.for_body(mass[0], sim.dt)
    sim.set_mooring((0.0, 0.0, -DEPTH), fairlead=(0.0, 0.0, -0.5), length=MOORING, stiffness=mk, damping=mc, bodies=[0])
    k, c = TetherNet.for_chain(mass, sim.dt)
    k *= 0.5 * STABLE / DEFAULT_K
    fair_a = np.zeros((n - 1, 3))
    fair_a[0] = (0.0, 0.0, -0.5)
    sim.set_tether_net(links=np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), fairlead_a=fair_a, layer=np.arange(n - 1) % 2,
                       length=LINK, stiffness=k, damping=c)
    peaks = sim.track_link_tensions()
    sim.run_resident(steps, chunk=min(chunk, steps))
    last, tension = sim.state().astype(np.float64), np.asarray(peaks.peak(), np.float64)
    sim.close()
    return last, tension


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3600)
    ap.add_argument("--chunk", type=int, default=600, help="physics steps per kernel launch")
    args = ap.parse_args(argv)

    sc = scene()
    tide = CurrentProfile.power_law(TIDE, 0.0, DEPTH, knots=12)
    wind = CurrentProfile.slab(WIND, WIND_HEADING, SLAB)
    profile = tide + wind
    surface = profile.velocity(0.0)
    uniform, peak_u = run(sc, SeaSpectrum(tuple(surface), depth=DEPTH), None, args.steps, args.chunk)
    sheared, peak_s = run(sc, SeaSpectrum(depth=DEPTH), profile, args.steps, args.chunk)
    heading = surface[0:2] / np.linalg.norm(surface[0:2])
    print(f"{args.steps} steps ({args.steps * sc.dt:.1f} s), surface current {np.linalg.norm(surface):.2f} m/s towards "
          f"{np.degrees(np.arctan2(surface[1], surface[0])):.0f} degrees in both runs; the profile: {TIDE} m/s tide (1/7 power law over {DEPTH:g} m) "
          f"+ {WIND} m/s wind slab over the top {SLAB:g} m towards {WIND_HEADING:g} degrees, {profile.knots} knots")
    print("current at the cable's bodies (m/s): " + "  ".join(f"{np.linalg.norm(profile.velocity(z)):.2f}" for z in sheared[:, 2]))
    for name, last in (("uniform", uniform), ("sheared", sheared)):
        print(f"cable shape, {name} (along the surface current, z): " + "  ".join(f"({p[0:2] @ heading:+.2f}, {p[2]:+.2f})" for p in last))
    for name, peak in (("uniform", peak_u), ("sheared", peak_s)):
        print(f"largest link tensions, {name} (N): " + " ".join(f"{t:.1f}" for t in np.ravel(peak)))
    off_u, off_s = float(uniform[-1, 0:2] @ heading), float(sheared[-1, 0:2] @ heading)
    across = float(sheared[-1, 0] * -heading[1] + sheared[-1, 1] * heading[0])
    print(f"ROV offset {off_u:6.2f} m uniform {off_s:6.2f} m sheared (along the surface current; {across:+.2f} m across it under the profile, which turns with depth)")
    if not (np.isfinite(uniform).all() and np.isfinite(sheared).all()):
        raise SystemExit("a run left the finite numbers")
    if not 0.0 < off_s < off_u:
        raise SystemExit("the sheared current did not carry the ROV less far than the uniform one")
    return {"uniform": uniform, "sheared": sheared}


if __name__ == "__main__":
    main()
