#!/usr/bin/env python3
"""What the seabed costs in the resident closed loop: hydro_step_fused_tiled_multi_bed with nobody near the bed, with everybody
resting on it, and with 8 wave components and a pose hold on top, against the loops that exist without it - the plain
resident loop (hydro_step_fused_tiled_multi), the pose-hold loop (_multi_ctl) and the current-only loop (_multi_sea).

  python scripts/diag_seabed.py              (GPU)  C2 buoys at 4 096, 19 456 and 1 048 576 bodies -> profiles/seabed.json
  python scripts/diag_seabed.py --isa-only   (no GPU) VALU and LDS instructions per step of the loops, registers, LDS and scratch
                                                     of the 32 instantiations, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows:
  plain          run_resident(chunk=64), still water, no bed
  ctl            set_pose_hold (a depth hold, kp = 25 m, kd = 10 m)
  sea_w0         set_sea(current only)
  bed_far        the scene as it is over a bed at z = -1000 m: nobody near it, every wave skips the contact
  bed_rest       every body as dense as rock, lying on the bed on four corners at its rest depth (its own start state)
  bed_w8_ctl     bed_far's bed, 8 wave components and the pose hold
Protocol (that of scripts/diag_sea.py): every timed window starts from the variant's initial state and step count 0, lasts at
least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per
physics step; bed_far and bed_rest over `plain`, bed_w8_ctl over `ctl`, and bed_far over bed_rest - the one expectation:
the far scene should cost visibly less than the resting one, or the broad phase is not working."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "seabed.json")
CHUNK = 64
SIZES = (4096, 19456, 1048576)
VARIANTS = ("plain", "ctl", "sea_w0", "bed_far", "bed_rest", "bed_w8_ctl")
KP, KD = 25.0, 10.0
Z_FAR, Z_REST = -1000.0, -5.0
KERNELS = ("step_fused_multi_tiled_kernel", "step_fused_multi_ctl_tiled_kernel", "step_fused_multi_sea_tiled_kernel",
           "step_fused_multi_bed_tiled_kernel")


def isa() -> dict:
    """Of the <f32, temporal, no KE, Numba> instantiations, per drag form: the instructions of the step loop, every branch of it
    counted (the bed loop holds the whole contact behind one scalar branch, the sea's eight component slots behind theirs,
    and each optional policy behind its own).  And over the 32 instantiations of the bed kernel: VGPRs, SGPRs, LDS bytes,
    scratch."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        row = {}
        for name in KERNELS:
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            # every basic block of the step loop: the header and the blocks annotated "in Loop" (the bed kernel's loop does not
            # begin with its header, so the span from the header to the back branch would miss part of it)
            blocks = re.split(r"^(\.LBB\d+_\d+:[^\n]*)\n", body, flags=re.M)
            loop = ops("\n".join(text for label, text in zip(blocks[1::2], blocks[2::2]) if "Loop" in label))
            row[name] = {"valu": sum(isa_mix.classify(op) != "not-valu" for op in loop),
                         "fp64": sum(isa_mix.classify(op) == "fp64 arithmetic" for op in loop),
                         "transcendental": sum(isa_mix.classify(op) == "transcendental" for op in loop),
                         "lds_reads": sum(op.startswith("ds_read") for op in loop), "lds_writes": sum(op.startswith("ds_write") for op in loop)}
        row["bed_valu_all_corners"] = row[KERNELS[3]]["valu"] - row[KERNELS[2]]["valu"]
        out["loop"][drag] = row
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if KERNELS[3] in m.group(1)}
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
    from scripts.diag_sea import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.seabed import Seabed
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        far, rest = Seabed.for_step(Z_FAR, sc.dt), Seabed.for_step(Z_REST, sc.dt)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        dev = sim.engine.device
        # the resting scene: the same bodies 2.5 times as dense as the water, upright, on the bed at their rest depth; the
        # engine's parameters are switched with the variant
        heavy = sc.params.copy()
        heavy[:, 10] = 2.5 * sc.rho * heavy[:, 0:3].prod(axis=1)
        lying = np.zeros_like(sc.state)
        lying[:, 0:2], lying[:, 6] = sc.state[:, 0:2], 1.0
        lying[:, 2] = Z_REST + 0.5 * heavy[:, 2] - rest.rest_depth(2.5, sc.g)
        starts = {"scene": (sim.cur.clone(), sim.old.clone()),
                  "lying": (torch.from_numpy(scenes.to_tiled(lying)).to(dev), torch.from_numpy(scenes.to_tiled(np.zeros_like(lying))).to(dev))}
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.synchronize()
            sim.engine.set_params(heavy if v == "bed_rest" else sc.params, sc.coeff_dtype)
            if v == "sea_w0" or v == "bed_w8_ctl":
                sim.set_sea(sea_of(0 if v == "sea_w0" else 8))
            else:
                sim.clear_sea()
            if v.endswith("ctl"):
                sim.set_pose_hold(position=sc.state[:, 0:3], kp_lin=np.concatenate([zero, zero, mass * KP], axis=1),
                                  kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
            else:
                sim.clear_pose_hold()
            if v.startswith("bed"):
                sim.set_seabed(rest if v == "bed_rest" else far)
            else:
                sim.clear_seabed()

        def window(v, steps):
            select(v)
            cur, old = starts["lying" if v == "bed_rest" else "scene"]
            with torch.cuda.stream(sim.stream):
                sim.cur.copy_(cur); sim.old.copy_(old)
            sim.steps_done = 0
            sim.synchronize()
            t0 = time.perf_counter()
            sim.run_resident(steps, chunk=CHUNK)
            sim.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6                              # us per physics step

        steps, touching = {}, {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                          # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                           # warm-up, discarded
            if v.startswith("bed"):
                probe = scenes.from_tiled(sim.engine.seabed_wrench(sim.cur, n).cpu().numpy(), n)
                touching[v] = float((probe[:, 2] > 0).mean())                             # share of the bodies on the bed at the end of a window
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "implicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "over_plain": {v: round(med[v] / med["plain"], 4) for v in ("ctl", "sea_w0", "bed_far", "bed_rest")},
               "bed_w8_ctl_over_ctl": round(med["bed_w8_ctl"] / med["ctl"], 4),
               "bed_far_over_bed_rest": round(med["bed_far"] / med["bed_rest"], 4),
               "share_touching_at_the_end_of_a_window": touching,
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
        data["protocol"] = (f"one sim per size, implicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the variant's initial state and step count 0, ending in a stream synchronise; variants alternate "
                            f"within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
