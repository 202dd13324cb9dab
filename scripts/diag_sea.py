#!/usr/bin/env python3
"""What moving water costs in the resident closed loop: hydro_step_fused_tiled_multi_sea with a current only and with 1, 4 and
8 regular wave components, against the loops that exist without it - the plain resident loop
(hydro_step_fused_tiled_multi) and the pose-hold loop (hydro_step_fused_tiled_multi_ctl).

  python scripts/diag_sea.py              (GPU)  C2 buoys at 4 096, 19 456 and 1 048 576 bodies -> profiles/sea_state.json
  python scripts/diag_sea.py --isa-only   (no GPU) VALU, transcendental, scalar-load and LDS instructions per step of the loops,
                                                  registers, LDS and scratch of the 32 instantiations, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows:
  plain        run_resident(chunk=64), still water
  ctl          set_pose_hold (a depth hold, kp = 25 m, kd = 10 m), still water
  sea_w0       set_sea(current only)          sea_w1 / sea_w4 / sea_w8: the current plus 1 / 4 / 8 wave components
  sea_w8_ctl   8 components and the pose hold
Protocol (that of scripts/diag_pose_hold.py): every timed window starts from the same initial state and step count, lasts at
least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per
physics step, and each sea variant over `plain` (sea_w8_ctl over `ctl`)."""
import argparse
import json
import math
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "sea_state.json")
CHUNK = 64
SIZES = (4096, 19456, 1048576)
VARIANTS = ("plain", "ctl", "sea_w0", "sea_w1", "sea_w4", "sea_w8", "sea_w8_ctl")
KP, KD = 25.0, 10.0
KERNELS = ("step_fused_multi_tiled_kernel", "step_fused_multi_ctl_tiled_kernel", "step_fused_multi_sea_tiled_kernel")


def sea_of(waves: int):
    """A 0.3 m/s current and `waves` components, wavelengths from 100 m down, headings fanned over 140 degrees."""
    from silver2_isaacsim_amd.sea import SeaState
    sea = SeaState((0.3, -0.1, 0.0))
    for j in range(waves):
        kappa = 2.0 * math.pi / (100.0 / (1.0 + 1.5 * j))
        head = math.radians(-70.0 + 20.0 * j)
        sea.add_wave(0.2 / (1 + j), kappa * math.cos(head), kappa * math.sin(head), math.sqrt(9.81 * kappa), 0.7 * j)
    return sea


def isa() -> dict:
    """Of the <f32, temporal, no KE, Numba> instantiations, per drag form: instructions in one trip through the step loop (the
    sea loop holds all eight component slots behind scalar branches: its count is that of 8 components plus the branches).
    And over the 32 instantiations of the sea kernel: VGPRs, SGPRs, LDS bytes, scratch."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        row = {}
        for name in KERNELS:
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            loops = re.findall(r"^(\.LBB\d+_\d+):[^\n]*Loop Header[^\n]*\n", body, re.M)
            start = body.index(loops[0] + ":")
            end = max(m.end() for m in re.finditer(r"^\s+s_c?branch\S* " + re.escape(loops[0]) + r"$", body, re.M))
            loop = ops(body[start:end])
            row[name] = {"valu": sum(isa_mix.classify(op) != "not-valu" for op in loop),
                         "fp64": sum(isa_mix.classify(op) == "fp64 arithmetic" for op in loop),
                         "transcendental": sum(isa_mix.classify(op) == "transcendental" for op in loop),
                         "scalar_loads": sum(op.startswith("s_load") for op in loop),
                         "lds_reads": sum(op.startswith("ds_read") for op in loop), "lds_writes": sum(op.startswith("ds_write") for op in loop),
                         "global_loads": sum(op.startswith("global_load") for op in loop)}
        row["sea_valu_8_components"] = row[KERNELS[2]]["valu"] - row[KERNELS[1]]["valu"]
        out["loop"][drag] = row
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if KERNELS[2] in m.group(1)}
    span = lambda key: [min(int(d[key]) for d in desc.values()), max(int(d[key]) for d in desc.values())]  # noqa: E731
    out["instantiations"] = {"count": len(desc), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    per = {}
    for name, d in desc.items():
        flags = re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        per["<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags)) + ">"] = {
            "vgprs": int(d["next_free_vgpr"]), "lds_bytes": int(d["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
    out["per_instantiation"] = dict(sorted(per.items()))
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    seas = {0: sea_of(0), 1: sea_of(1), 4: sea_of(4), 8: sea_of(8)}
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        sim = ClosedLoopSim(sc)
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            if v.startswith("sea"):
                sim.set_sea(seas[int(re.search(r"w(\d)", v).group(1))])
            else:
                sim.clear_sea()
            if v.endswith("ctl"):
                sim.set_pose_hold(position=sc.state[:, 0:3], kp_lin=np.concatenate([zero, zero, mass * KP], axis=1),
                                  kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
            else:
                sim.clear_pose_hold()

        def window(v, steps):
            select(v)
            with torch.cuda.stream(sim.stream):
                sim.cur.copy_(start[0]); sim.old.copy_(start[1])
            sim.steps_done = 0
            sim.synchronize()
            t0 = time.perf_counter()
            sim.run_resident(steps, chunk=CHUNK)
            sim.synchronize()
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
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "explicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "over_plain": {v: round(med[v] / med["plain"], 4) for v in VARIANTS if v.startswith("sea") and not v.endswith("ctl")},
               "sea_w8_ctl_over_ctl": round(med["sea_w8_ctl"] / med["ctl"], 4),
               "final_state_finite": bool(torch.isfinite(sim.cur).all())}
        print(json.dumps(row), flush=True)
        results.append(row)
        sim.close()
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
        data["protocol"] = (f"one sim per size, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= {args.window} s from "
                            f"the same initial state and step count, ending in a stream synchronise; variants alternate within each of {args.rounds} "
                            f"rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
