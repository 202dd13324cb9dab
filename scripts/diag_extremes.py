#!/usr/bin/env python3
"""What the running extremes cost in the resident closed loop: hydro_step_fused_tiled_multi_ext with the record alone, with
everybody on a taut line, and with 8 wave components, a pose hold and a bed on top, against the loops that exist without the
record - the plain resident loop (hydro_step_fused_tiled_multi) and the mooring loop (_multi_moor), whose kernels this feature
leaves byte-identical: the baseline, measured in the same run.

  python scripts/diag_extremes.py              (GPU)  C2 buoys at 4 096, 19 456 and 1 048 576 bodies -> profiles/extremes.json
  python scripts/diag_extremes.py --isa-only   (no GPU) VALU and LDS instructions per step of the loops, registers, LDS and scratch
                                                      of the 32 instantiations, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows:
  plain               run_resident(chunk=64), still water
  ext                 track_extremes() and nothing else: the new kernel with every option absent
  moor_taut           every body on a line of its own, 4.9 m of line to an anchor 5 m below it, the default constants for its mass
  ext_moor_taut       the same with the record
  moor_w8_ctl_bed     the lines, 8 wave components, a depth hold and a bed at z = -1000 m
  ext_moor_w8_ctl_bed the same with the record
Protocol (that of scripts/diag_mooring.py): every timed window starts from the same initial state and step count 0, lasts at
least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per
physics step; ext over plain, ext_moor_taut over moor_taut and ext_moor_w8_ctl_bed over moor_w8_ctl_bed.  No ratio is fixed in
advance; the one expectation: four paired LDS reads, four paired LDS writes and about twenty VALU instructions per step
should be small against the full loop's 1 500 to 1 900."""

import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "extremes.json")
CHUNK = 64
SIZES = (4096, 19456, 1048576)
VARIANTS = ("plain", "ext", "moor_taut", "ext_moor_taut", "moor_w8_ctl_bed", "ext_moor_w8_ctl_bed")
PAIRS = (("ext", "plain"), ("ext_moor_taut", "moor_taut"), ("ext_moor_w8_ctl_bed", "moor_w8_ctl_bed"))
KP, KD = 25.0, 10.0
Z_FAR = -1000.0
KERNELS = ("step_fused_multi_tiled_kernel", "step_fused_multi_moor_tiled_kernel", "step_fused_multi_ext_tiled_kernel")


def isa() -> dict:
    """Of the <f32, temporal, no KE, Numba> instantiations, per drag form: the instructions of the step loop, every branch of it
    counted (each optional policy stands behind a scalar branch of its own; the extremes' update behind none).  And over the
    32 instantiations of the extremes kernel: VGPRs, SGPRs, LDS bytes, scratch - each of them listed."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        row = {}
        for name in KERNELS:
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            blocks = re.split(r"^(\.LBB\d+_\d+:[^\n]*)\n", body, flags=re.M)
            loop = ops("\n".join(text for label, text in zip(blocks[1::2], blocks[2::2]) if "Loop" in label))
            row[name] = {"valu": sum(isa_mix.classify(op) != "not-valu" for op in loop),
                         "fp64": sum(isa_mix.classify(op) == "fp64 arithmetic" for op in loop),
                         "transcendental": sum(isa_mix.classify(op) == "transcendental" for op in loop),
                         "lds_reads": sum(op.startswith("ds_read") for op in loop), "lds_writes": sum(op.startswith("ds_write") for op in loop)}
        row["extremes_over_mooring"] = {k: row[KERNELS[2]][k] - row[KERNELS[1]][k] for k in ("valu", "lds_reads", "lds_writes")}
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
    from scripts.diag_sea import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import Mooring
    from silver2_isaacsim_amd.seabed import Seabed
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        far = Seabed.for_step(Z_FAR, sc.dt)
        k, c = Mooring.for_body(mass[:, 0], sc.dt)
        anchors = sc.state[:, 0:3].astype(np.float64) - np.array([0.0, 0.0, 5.0])
        sim = ClosedLoopSim(sc, implicit_drag=True)
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.synchronize()
            if v.endswith("w8_ctl_bed"):
                sim.set_sea(sea_of(8))
            else:
                sim.clear_sea()
            if "ctl" in v:
                sim.set_pose_hold(position=sc.state[:, 0:3], kp_lin=np.concatenate([zero, zero, mass * KP], axis=1),
                                  kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
            else:
                sim.clear_pose_hold()
            if "bed" in v:
                sim.set_seabed(far)
            else:
                sim.clear_seabed()
            if "moor" in v:
                sim.set_mooring(anchors, length=4.9, stiffness=k, damping=c)
            else:
                sim.clear_mooring()
            if v.startswith("ext"):
                sim.track_extremes()
            else:
                sim.clear_extremes()

        def window(v, steps):
            select(v)
            with torch.cuda.stream(sim.stream):
                sim.cur.copy_(start[0]); sim.old.copy_(start[1])
            sim.steps_done = 0
            if sim.extremes is not None:
                sim.extremes.reset()
            sim.synchronize()
            t0 = time.perf_counter()
            sim.run_resident(steps, chunk=CHUNK)
            sim.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6                              # us per physics step

        steps, pulling, peak = {}, {}, {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                          # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                           # warm-up, discarded
            if v.startswith("ext"):
                peak[v] = float(sim.extremes.tension_max().max())                         # the record at the end of a window: the largest tension
            if "moor" in v:
                probe = scenes.from_tiled(sim.engine.mooring_wrench(sim.cur, sim.mooring, n).cpu().numpy(), n)
                pulling[v] = float(probe.any(axis=1).mean())                              # share of the bodies whose line pulls at the end of a window
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "implicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "with_extremes_over_without": {f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in PAIRS},
               "share_pulling_at_the_end_of_a_window": pulling, "largest_tension_max_at_the_end_of_a_window": peak,
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
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["loop"]))
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"one sim per size, implicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the same initial state and step count 0, ending in a stream synchronise; variants alternate "
                            f"within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
