#!/usr/bin/env python3
"""Closed-loop CONTROL on the fast path: a few thousand neutrally buoyant boxes ("ROVs"), each holding its own depth
set-point with a PD law - the job of the reference's robot.py / cmd_vel layer, where PhysX applies the thruster forces.
Here the library is the integrator, so the thrust goes into the stepping kernel as an applied wrench:

  * the bodies are stepped `chunk` steps per launch, resident in registers (ClosedLoopSim.run_resident);
  * between two launches the controller - a handful of torch operations on `sim.stream` - reads depth, vertical velocity
    and attitude from the tiled state and writes the next command into `sim.applied`, the buffer the kernel reads: a thrust
    in the BODY frame (a vehicle's thrusters turn with it), which the kernel turns back with the attitude of every step;
  * nothing goes through the host: the only synchronisation is the one at the end.

    python examples/rov_depth_hold.py --bodies 4096 --steps 600
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402

KP, KD = 25.0, 10.0          # per unit mass: 5 rad/s, critically damped before the water adds its own damping


def rov_scene(n: int, seed: int = 0):
    """n neutrally buoyant boxes (mass = rho * volume) at rest, 3 .. 8 m deep, tilted by a few degrees, and the depth each
    is to hold: up to 1 m above or below where it starts."""
    rng = np.random.default_rng(seed)
    dims = rng.uniform(0.3, 0.8, (n, 3))
    q = np.concatenate([rng.normal(0.0, 0.05, (n, 3)), np.ones((n, 1))], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    pos = np.concatenate([rng.uniform(-50.0, 50.0, (n, 2)), rng.uniform(-8.0, -3.0, (n, 1))], axis=1)
    state = np.concatenate([pos, q, np.zeros((n, 6))], axis=1).astype(np.float32)
    coeffs = scenes._DEFAULT_COEFFS[None, :] * rng.uniform(0.8, 1.2, (n, 7))
    params = np.concatenate([dims, coeffs, (scenes.RHO * dims.prod(axis=1))[:, None]], axis=1).astype(np.float32)
    setpoint = (state[:, 2] + rng.uniform(0.3, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return scenes.Scene("ROV depth hold", state, np.zeros((n, 6), np.float32), params), setpoint


def depth_command(state: torch.Tensor, setpoint: torch.Tensor, mass: torch.Tensor, out: torch.Tensor) -> None:
    """The PD law on tiled tensors: state (tiles, 13, 64), setpoint and mass (tiles, 64) -> out (tiles, 6, 64), the thrust
    u = m (kp (z* - z) - kd v_z) along world z, expressed in the body frame: R^T (0, 0, u) = u * (third row of R)."""
    u = mass * (KP * (setpoint - state[:, 2]) - KD * state[:, 9])
    x, y, z, w = state[:, 3], state[:, 4], state[:, 5], state[:, 6]
    out[:, 0] = u * 2.0 * (x * z - w * y)
    out[:, 1] = u * 2.0 * (y * z + w * x)
    out[:, 2] = u * (1.0 - 2.0 * (x * x + y * y))


def main(steps: int = 600, bodies: int = 4096, chunk: int = 4, control: bool = True, seed: int = 0) -> dict:
    scene, setpoint = rov_scene(bodies, seed)
    # implicit drag: the angular damping of a 0.3 m box is past what the explicit form holds at 60 Hz (|k| dt / I > 2)
    sim = ClosedLoopSim(scene, implicit_drag=True)
    dev = sim.engine.device
    pad = sim.cur.shape[0] * 64 - bodies
    as_tiled = lambda a: torch.from_numpy(np.concatenate([a, np.zeros(pad, np.float32)]).reshape(-1, 64)).to(dev)  # noqa: E731
    target, mass = as_tiled(setpoint), as_tiled(scene.params[:, 10])
    sim.set_applied_wrench(np.zeros((bodies, 6), np.float32), frame="body")
    sim.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(chunk, steps - done)
        if control:
            with torch.cuda.stream(sim.stream):
                depth_command(sim.cur, target, mass, sim.applied)         # the next command, on the device
        sim.run_resident(k, chunk=k)
        done += k
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
    ap.add_argument("--chunk", type=int, default=4, help="physics steps per launch = per controller update")
    args = ap.parse_args()
    for on in (False, True):
        r = main(args.steps, args.bodies, args.chunk, control=on)
        print(f"controller {'on ' if on else 'off'}: mean |z* - z| {r['start_error']:.3f} m -> {r['depth_error']:.4f} m "
              f"(max {r['max_depth_error']:.4f} m) after {args.steps} steps; {r['us_per_step']:.2f} us per step, RTF {r['rtf']:.0f} x")
