#!/usr/bin/env python3
"""What a controller at the rate of the physics costs: the pose hold inside the resident loop
(hydro_step_fused_tiled_multi_ctl) against the plain resident loop and against the only way to the same control rate
without it - one launch per step with the law in torch between the launches.

  python scripts/diag_pose_hold.py              (GPU)  C2 buoys at 4 096, 19 456 and 1 048 576 bodies, explicit and implicit
                                                       drag -> profiles/pose_hold.json
  python scripts/diag_pose_hold.py --isa-only   (no GPU) VALU and LDS instructions per step of the loops, registers and LDS of
                                                       the 32 instantiations, from hipcc -S

Variants of a (size, drag) pair - sims of the same scene, each body holding the depth it starts at (kp = 25 m, kd = 10 m):
  plain   run_resident(chunk=64), no controller
  outer   hydro_step_fused_tiled_multi_app at chunk = 1, the PD law as torch operations on the step stream before every launch
  hold    set_pose_hold, run_resident(chunk=64)
Protocol (that of scripts/diag_applied.py): every timed window starts from the same initial state, lasts at least --window
seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of --rounds rounds,
after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per physics step."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "pose_hold.json")
CHUNK = 64
SIZES = (4096, 19456, 1048576)
VARIANTS = ("plain", "outer", "hold")
KP, KD = 25.0, 10.0
KERNELS = ("step_fused_multi_tiled_kernel", "step_fused_multi_app_tiled_kernel", "step_fused_multi_ctl_tiled_kernel")


def isa() -> dict:
    """Per drag form, of the <f32, temporal, no KE, Numba> instantiations: VALU and LDS instructions in one trip through the
    step loop (the applied and the pose-hold loop hold both frames of the applied wrench behind one scalar branch; the
    difference of the two is the law with its LDS reads).  And over the 32 instantiations of the pose-hold kernel: VGPRs,
    SGPRs, LDS bytes, scratch."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        row = {}
        for name in KERNELS:
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            loop = ops(re.search(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)^\s+s_branch \1$", body, re.S | re.M).group(2))
            row[name] = {"valu": sum(isa_mix.classify(op) != "not-valu" for op in loop), "lds_reads": sum(op.startswith("ds_read") for op in loop),
                         "global_loads": sum(op.startswith("global_load") for op in loop)}
        row["law_valu"] = row[KERNELS[2]]["valu"] - row[KERNELS[1]]["valu"]
        out["loop"][drag] = row
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if KERNELS[2] in m.group(1)}
    span = lambda key: [min(int(d[key]) for d in desc.values()), max(int(d[key]) for d in desc.values())]  # noqa: E731
    out["instantiations"] = {"count": len(desc), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        for implicit in (False, True):
            sims = {v: ClosedLoopSim(sc, implicit_drag=implicit) for v in VARIANTS}
            sims["hold"].set_pose_hold(kp_lin=np.concatenate([zero, zero, mass * KP], axis=1), kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
            outer = sims["outer"]
            outer.set_applied_wrench(np.zeros((n, 6), np.float32), frame="world")
            dev = outer.engine.device
            m_t = torch.from_numpy(scenes.to_tiled(sc.params[:, 10:11])).to(dev)[:, 0]
            z_t = torch.from_numpy(scenes.to_tiled(sc.state[:, 2:3])).to(dev)[:, 0]
            start = {v: (s.cur.clone(), s.old.clone()) for v, s in sims.items()}

            def run(v, steps):
                s = sims[v]
                if v != "outer":
                    s.run_resident(steps, chunk=CHUNK)
                    return
                for _ in range(steps):
                    with torch.cuda.stream(s.stream):                                         # the law, between the launches
                        s.applied[:, 2] = m_t * (KP * (z_t - s.cur[:, 2]) - KD * s.cur[:, 9])
                    s.run_resident(1, chunk=1)

            def window(v, steps):
                s = sims[v]
                with torch.cuda.stream(s.stream):
                    s.cur.copy_(start[v][0]); s.old.copy_(start[v][1])
                s.synchronize()
                t0 = time.perf_counter()
                run(v, steps)
                s.synchronize()
                return (time.perf_counter() - t0) / steps * 1e6                              # us per physics step

            steps = {}
            for v in VARIANTS:
                window(v, 2 * CHUNK)                                                          # (first launches: code objects, clocks)
                steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
                window(v, steps[v])                                                           # warm-up, discarded
            times = {v: [] for v in VARIANTS}
            for _ in range(rounds):
                for v in VARIANTS:
                    times[v].append(window(v, steps[v]))
            finite = {v: bool(torch.isfinite(s.cur).all()) for v, s in sims.items()}
            med = {v: statistics.median(t) for v, t in times.items()}
            row = {"bodies": n, "drag": "implicit" if implicit else "explicit", "chunk": {"plain": CHUNK, "outer": 1, "hold": CHUNK},
                   "steps_per_window": steps, "rounds": rounds,
                   "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
                   "hold_over_plain": round(med["hold"] / med["plain"], 4), "hold_over_outer": round(med["hold"] / med["outer"], 4),
                   "final_state_finite": finite}
            print(json.dumps(row), flush=True)
            results.append(row)
            for s in sims.values():
                s.close()
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa-only", action="store_true", help="count instructions only (no GPU)")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.isa_only:
        data["isa"] = isa()
        print(json.dumps(data["isa"]))
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"plain / hold: run_resident(chunk={CHUNK}); outer: one applied launch per step with the torch PD law before it; windows "
                            f"of >= {args.window} s from the same initial state, ending in a stream synchronise; variants alternate within each of "
                            f"{args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
