#!/usr/bin/env python3
"""Boxes on the seabed: a few thousand boxes denser than water - four shapes from a 1 m cube barely heavier than the water to a
steel-dense plate, released flat, tilted and on an edge 1 m above a bed at z = -5 m with a little forward speed - sink, land,
slide to a halt and rest on four corners.  The bed lives inside the stepping kernel (`ClosedLoopSim.set_seabed`): every
physics step meets it while the bodies stay resident in registers, one launch per `--chunk` steps.  The script prints how
many boxes are at rest and how their rest depth compares with the analytic one, g (1 - rho / rho_body) / (4 kappa) below the
plane.

    python examples/boxes_on_seabed.py --boxes 4096 --steps 720 --chunk 240
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.seabed import Seabed                        # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

Z_BED = -5.0
BOXES = (((0.5, 0.5, 0.5), 2.0), ((1.0, 1.0, 1.0), 1.05), ((0.8, 0.3, 0.2), 1.3), ((0.3, 0.2, 0.1), 7.8))      # dimensions (m), rho_body / rho


def _about(axis, angle):
    q = np.zeros(4)
    q[axis], q[3] = np.sin(angle / 2), np.cos(angle / 2)
    return q


def _times(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


ATTITUDES = (_about(0, 0.0), _times(_about(1, 0.35), _about(0, 0.5)), _about(0, np.pi / 4))       # flat, tilted, on an edge


def scene(n: int, dt: float) -> tuple:
    """n boxes on a grid 3 m apart, cycling through the four boxes and the three attitudes; returns (Scene, rho_body / rho)."""
    state = np.zeros((n, 13), np.float32)
    params = np.zeros((n, 11), np.float32)
    ratios = np.zeros(n)
    side = int(np.ceil(np.sqrt(n)))
    for i in range(n):
        dims, ratio = BOXES[i % len(BOXES)]
        state[i, 0:3] = (3.0 * (i % side), 3.0 * (i // side), Z_BED + 1.0)
        state[i, 3:7] = ATTITUDES[(i // len(BOXES)) % len(ATTITUDES)]
        state[i, 7] = 0.3
        params[i] = np.concatenate([dims, scenes._DEFAULT_COEFFS, [ratio * scenes.RHO * np.prod(dims)]])
        ratios[i] = ratio
    return scenes.Scene("boxes on the seabed", state, np.zeros((n, 6), np.float32), params, dt=dt), ratios


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=720, help="physics steps (12 s at 60 Hz)")
    ap.add_argument("--chunk", type=int, default=240, help="physics steps per kernel launch")
    ap.add_argument("--rate", type=int, default=60, help="physics steps per second")
    args = ap.parse_args(argv)

    dt = float(np.float32(1.0 / args.rate))
    sc, ratios = scene(args.boxes, dt)
    bed = Seabed.for_step(Z_BED, dt)
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_seabed(bed)
    sim.run_resident(args.steps, chunk=args.chunk)
    final = sim.state().astype(np.float64)
    sim.close()

    below = bed.z - (final[:, None, 2] + bed.corners(final, sc.params)[:, :, 2])                 # (n, 8) penetrations
    speed, spin = np.linalg.norm(final[:, 7:10], axis=1), np.linalg.norm(final[:, 10:13], axis=1)
    resting = ((below > 0).sum(axis=1) == 4) & (speed < 1e-4) & (spin < 1e-4)
    analytic = np.array([bed.rest_depth(r, sc.g) for r in ratios])
    print(f"{args.boxes} boxes, {args.steps} steps of 1/{args.rate} s in launches of {args.chunk}; bed at z = {bed.z:g} m, "
          f"kappa = {bed.stiffness:g} / s^2, beta = gamma = {bed.damping:g} / s, mu = {bed.friction:g}")
    print(f"at rest on four corners: {int(resting.sum())} of {args.boxes}  (|v| <= {speed.max():.2e} m/s, |omega| <= {spin.max():.2e} rad/s)")
    slid = final[:, 0] - sc.state[:, 0]
    print(f"slid {slid.min():.2f} .. {slid.max():.2f} m along x before stopping")
    print(f"rest depth against g (1 - rho / rho_body) / (4 kappa): largest difference {np.abs(below.max(axis=1) - analytic).max():.2e} m "
          f"(depths {1e3 * analytic.min():.2f} .. {1e3 * analytic.max():.2f} mm)")
    return {"resting": int(resting.sum()), "depth_error": float(np.abs(below.max(axis=1) - analytic).max())}


if __name__ == "__main__":
    main()
