#!/usr/bin/env python3
"""The reference's validation artefact from the FAST path: config 1's buoy (hydrodynamics of one floating cube, released
above its equilibrium) stepped 10 000 times with the body resident in registers - ten kernel launches - while a trajectory
recorder writes its pose and velocity after EVERY step from inside those launches.  The log becomes the reference's
`velocity_log.csv` (log_velocity.py: same header, same (z, x, y) column order), one row per physics step, without one host
round trip per row; the real-time factor is printed with and without the recorder attached.

    python examples/buoy_trajectory_resident.py --steps 10000 --chunk 1000 --out /tmp/demo
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes                               # noqa: E402
from silver2_isaacsim_amd.simulate import ClosedLoopSim               # noqa: E402
from silver2_isaacsim_amd.telemetry import write_velocity_log         # noqa: E402


def timed(sim, steps, chunk, recorder=None):
    """measure_rtf for a run that may record: the log is rewound before the warm-up launch and before the timed run."""
    for k in (chunk, steps):
        if recorder is not None:
            recorder.rewind()
        sim.synchronize()
        t0 = time.perf_counter()
        sim.run_resident(k, chunk)
        sim.synchronize()
        wall = time.perf_counter() - t0
    return {"rtf": steps * sim.dt / wall, "us_per_step": wall / steps * 1e6}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=1000, help="physics steps per kernel launch")
    ap.add_argument("--every", type=int, default=1, help="record every N-th step")
    ap.add_argument("--out", default=".")
    args = ap.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)

    # the artefact: one run from the initial state, every `every`-th step recorded
    sim = ClosedLoopSim(scenes.scene_c1())
    rec = sim.record([0], every=args.every, rows=args.steps // args.every + 1)
    sim.run_resident(args.steps, chunk=args.chunk)
    path = write_velocity_log(args.out, rec, 0, start=datetime.datetime.now(), dt=sim.dt)
    z = rec.states()[:, 0, 2]
    print(f"{len(z)} rows -> {path}")
    print(f"buoy z: start {scenes.scene_c1().state[0, 2]:+.4f} m, min {z.min():+.4f}, max {z.max():+.4f}, "
          f"last {z[-1]:+.4f} m after {rec.steps()[-1]} steps ({rec.steps()[-1] * sim.dt:.1f} s)")
    if args.steps % args.every == 0:                              # the last row IS the state the run ended in
        assert np.array_equal(rec.states()[-1, 0], sim.state()[0])

    # what the recorder costs: the same loop with and without it
    with_rec = timed(sim, args.steps, args.chunk, rec)
    sim.stop_recording()
    without = timed(sim, args.steps, args.chunk)
    print(f"RTF with the recorder:    {with_rec['rtf']:10.0f} x   ({with_rec['us_per_step']:.3f} us per step)")
    print(f"RTF without the recorder: {without['rtf']:10.0f} x   ({without['us_per_step']:.3f} us per step)")
    sim.close()
    return {"csv": path, "rows": len(z), "rtf_recorded": with_rec["rtf"], "rtf_plain": without["rtf"]}


if __name__ == "__main__":
    main()
