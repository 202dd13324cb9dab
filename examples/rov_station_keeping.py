#!/usr/bin/env python3
"""Closed-loop control INSIDE the fast path: the scene of examples/rov_depth_hold.py - a few thousand neutrally buoyant
boxes, each holding its own depth set-point - with the PD law evaluated by the stepping kernel itself.

rov_depth_hold.py closes the loop between launches: one launch per `chunk` steps, a handful of torch kernels before each,
and a command that is `chunk` steps old by the end of a launch - so it runs at chunk = 4.  Here the law is the pose hold
(ClosedLoopSim.set_pose_hold -> hydro_step_fused_tiled_multi_ctl): it sees the state of EVERY step while the bodies stay
resident in registers, so the controller runs at the rate of the physics and `chunk` is free again: 64 steps per launch,
nothing between the launches, nothing through the host.

  * kp_lin = (0, 0, m KP), kd_lin = (0, 0, m KD): a pure depth hold - the horizontal axes are left alone;
  * --attitude adds a hold of the upright attitude (kp_ang, kd_ang scaled by the box's inertia);
  * the set-points live in `sim.control`; a planner on the device may move them between chunks.

    python examples/rov_station_keeping.py --bodies 4096 --steps 600
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rov_depth_hold import KD, KP, rov_scene                           # noqa: E402  (the same scene, the same gains)
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402


def main(steps: int = 600, bodies: int = 4096, chunk: int = 64, control: bool = True, attitude: bool = False, seed: int = 0) -> dict:
    scene, setpoint = rov_scene(bodies, seed)
    sim = ClosedLoopSim(scene, implicit_drag=True)                        # (implicit drag: see rov_depth_hold.py)
    if control:
        mass = scene.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        target = scene.state[:, 0:3].copy()
        target[:, 2] = setpoint
        hold = dict(position=target, kp_lin=np.concatenate([zero, zero, mass * KP], axis=1), kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
        if attitude:
            inertia = mass[:, 0] / 12.0 * (scene.params[:, 0:3].astype(np.float64) ** 2).sum(axis=1)    # (an upper bound of the three moments)
            hold.update(orientation_xyzw=(0.0, 0.0, 0.0, 1.0), kp_ang=inertia * KP, kd_ang=inertia * KD)
        sim.set_pose_hold(**hold)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_resident(steps, chunk=chunk)
    state = sim.state()                                                   # the one host synchronisation
    wall = time.perf_counter() - t0
    sim.close()
    error = np.abs(state[:, 2].astype(np.float64) - setpoint)
    return {"state": state, "setpoint": setpoint, "depth_error": float(error.mean()), "max_depth_error": float(error.max()),
            "start_error": float(np.abs(scene.state[:, 2].astype(np.float64) - setpoint).mean()),
            "rtf": steps * scene.dt / wall, "us_per_step": wall / steps * 1e6}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--bodies", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=64, help="physics steps per launch; the controller acts at every step whatever this is")
    ap.add_argument("--attitude", action="store_true", help="also hold the upright attitude")
    args = ap.parse_args()
    for on in (False, True):
        r = main(args.steps, args.bodies, args.chunk, control=on, attitude=args.attitude)
        print(f"pose hold {'on ' if on else 'off'}: mean |z* - z| {r['start_error']:.3f} m -> {r['depth_error']:.4f} m "
              f"(max {r['max_depth_error']:.4f} m) after {args.steps} steps; {r['us_per_step']:.2f} us per step, RTF {r['rtf']:.0f} x")
