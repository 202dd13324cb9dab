#!/usr/bin/env python3
"""What the response statistics cost in the resident closed loop: hydro_step_fused_tiled_multi_stat - four fp64 sums and two
up-crossing words per body, parked in LDS and updated behind the integrator in every step - against the kernels this feature
leaves byte-identical, measured in the same run.

  python scripts/diag_statistics.py              (GPU)  C2 buoys at 4 096 and 1 048 576 bodies -> profiles/statistics.json
  python scripts/diag_statistics.py --isa-only   (no GPU) registers, LDS and scratch of the 64 instantiations and the instructions
                                                          the policy adds to the step loop, from hipcc -S (--asm FILE: a listing at hand)

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, explicit drag:
  sea8_spread_ext          a regular sea of 8 components, a three-line spread and the extremes: the parent's spread kernel
  sea8_spread_ext_stat     the same with track_statistics(("z", "tension")): the _stat kernel
  irr64_spread_ext         64 components with the same spread and extremes: the parent's _irr kernel
  irr64_spread_ext_stat    the same with track_statistics: the _irr_stat kernel
Protocol (that of scripts/diag_extremes.py and scripts/diag_sea_spectrum.py): every timed window starts from the same initial
state and step count 0 with the records reset, lasts at least --window seconds of back-to-back launches of run_resident(chunk=64)
and ends in a stream synchronise; the variants alternate within each of --rounds rounds, after a warm-up window each.  Reported:
the median over the rounds and the range, in us per physics step.  No ratio is gated.  The expectation written down beforehand is
EXPECTATION."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "statistics.json")
CHUNK = 64
SIZES = (4096, 1048576)
VARIANTS = ("sea8_spread_ext", "sea8_spread_ext_stat", "irr64_spread_ext", "irr64_spread_ext_stat")
PAIRS = (("sea8_spread_ext_stat", "sea8_spread_ext"), ("irr64_spread_ext_stat", "irr64_spread_ext"))
FAMILIES = {"step_fused_multi_stat_tiled_kernel": "step_fused_multi_spread_tiled_kernel",
            "step_fused_multi_irr_stat_tiled_kernel": "step_fused_multi_irr_tiled_kernel"}
EXPECTATION = ("per step and body the policy adds about 8 fp64 instructions (two conversions, a subtraction, two additions and a product per "
               "channel, less what the two channels share), a dozen fp32 / integer ones (the channel selects, the compares, the word update), "
               "four 8-byte LDS reads and writes and two 4-byte ones, and 8 B of global read that hits in L2 after the first step - against a "
               "step loop of 1 500 instructions or more (the spread kernel with a sea of 8 components; several times that with 64).  Where the "
               "loop is bound by VALU issue that is 2 - 3 % on the regular sea and under 1 % on the spectrum; the LDS traffic rides in the "
               "shadow of the fp64 wrench.  The 10 240 B of LDS per block do not cost the third block of a CU (53 248 B <= 54 613 B).  Per "
               "launch the record adds 44 B read and 44 B written per body: at chunk = 64 that is 1.4 B per body-step beside the 3 B the state "
               "costs, visible only where the launch is memory-bound, which a chunk of 64 steps is not")


def isa(asm_path=None) -> dict:
    """Over the 2 x 32 instantiations: VGPRs, SGPRs, LDS bytes and scratch beside the instantiation of the same flags of the family
    each is built on, and the instructions the policy adds to the step loop (the outermost loop of the kernel)."""
    from scripts import isa_mix
    asm = open(asm_path).read() if asm_path else isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    kind = lambda op, what: isa_mix.classify(op) == what  # noqa: E731
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}

    def step_loop(kernel, flags="ILb0ELb0ELb0ELb0ELb0E"):
        body = re.search(r"^(_Z\S*\d" + kernel + flags + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
        # the blocks of the step loop - the kernel's only loop of depth 1 - and of the loops inside it, wherever the layout put them:
        # a block's label carries, as a comment, the loop it belongs to
        labels = list(re.finditer(r"^\.LBB\d+_\d+:[^\n]*\n(?:\s*;[^\n]*\n)*", body, re.M))
        best = []
        for m, nxt in zip(labels, labels[1:] + [None]):
            if re.search(r"Depth=[12]|Loop BB\d+_\d+ Depth", m.group(0)):
                best += ops(body[m.end():nxt.start() if nxt else len(body)])
        return {"instructions": len(best), "valu": sum(not kind(op, "not-valu") for op in best), "fp64": sum(kind(op, "fp64 arithmetic") for op in best),
                "lds": sum(op.startswith("ds_") for op in best), "global_memory": sum(op.startswith("global_") for op in best),
                "scratch": sum(op.startswith("scratch_") for op in best)}
    out = {"step_loop": {}}
    for new, base in FAMILIES.items():
        a, b = step_loop(new), step_loop(base)
        out["step_loop"][new] = {"with": a, "built_on": b, "added": {k: a[k] - b[k] for k in a}}
    per, ok = {}, True
    for new, base in FAMILIES.items():
        mine = {flags_of(k): d for k, d in desc.items() if re.search(r"\d" + new + "I", k)}
        theirs = {flags_of(k): d for k, d in desc.items() if re.search(r"\d" + base + "I", k)}
        ok = ok and len(mine) == 32
        for flags, d in sorted(mine.items()):
            vgprs = int(d["next_free_vgpr"])
            row = {"vgprs": vgprs, "built_on_vgprs": int(theirs[flags]["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
                   "waves_per_simd": 512 // (-(-vgprs // 8) * 8), "lds_bytes": int(d["group_segment_fixed_size"]),
                   "built_on_lds_bytes": int(theirs[flags]["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
            ok = ok and row["scratch_bytes"] == 0 and vgprs <= 168 and row["lds_bytes"] <= 54613 and row["lds_bytes"] == row["built_on_lds_bytes"] + 10240
            per[new + "<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags)) + ">"] = row
    span = lambda key: [min(v[key] for v in per.values()), max(v[key] for v in per.values())]  # noqa: E731
    out["instantiations"] = {"count": len(per), "vgprs": span("vgprs"), "sgprs": span("sgprs"), "lds_bytes": span("lds_bytes"), "scratch_bytes": span("scratch_bytes"),
                             "lds_limit_for_three_blocks": 54613}
    out["per_instantiation"] = per
    reset = [d for k, d in desc.items() if "statistics_reset_kernel" in k]
    out["reset_kernel"] = {"vgprs": int(reset[0]["next_free_vgpr"]), "lds_bytes": int(reset[0]["group_segment_fixed_size"]), "scratch_bytes": int(reset[0]["private_segment_fixed_size"])}
    out["conditions_met"] = bool(ok)
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from scripts.diag_sea_spectrum import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import MooringSpread
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    seas = {"sea8": sea_of(8, False), "irr64": sea_of(64, True)}
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10].astype(np.float64)
        pos = sc.state[:, 0:3].astype(np.float64)
        k, c = MooringSpread.for_body(mass, sc.dt, 3)
        phi = 2.0 * np.pi * np.arange(3) / 3.0
        anchors = np.stack([pos[:, None, 0] + 6.0 * np.cos(phi)[None, :], pos[:, None, 1] + 6.0 * np.sin(phi)[None, :],
                            np.broadcast_to(pos[:, None, 2] - 8.0, (n, 3))], axis=2)                # reach 10 m; 9.9 m of line: taut
        sim = ClosedLoopSim(sc)
        start = (sim.cur.clone(), sim.old.clone())
        sim.set_mooring_spread(anchors=anchors, length=9.9, stiffness=np.repeat(k[:, None], 3, axis=1), damping=np.repeat(c[:, None], 3, axis=1))
        sim.track_extremes()
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.set_sea(seas[v.split("_")[0]])
            if v.endswith("_stat"):
                sim.track_statistics(("z", "tension"))
            else:
                sim.clear_statistics()

        def window(v, steps):
            select(v)
            with torch.cuda.stream(sim.stream):
                sim.cur.copy_(start[0]); sim.old.copy_(start[1])
            sim.steps_done = 0
            sim.extremes.reset()
            if sim.statistics is not None:
                sim.statistics.reset()
            sim.synchronize()
            t0 = time.perf_counter()
            sim.run_resident(steps, chunk=CHUNK)
            sim.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6                                  # us per physics step

        steps = {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                              # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                               # warm-up, discarded
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        counted = sim._statistics_view.count()
        row = {"bodies": n, "drag": "explicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "ratios": {f"{a_}_over_{b_}": round(med[a_] / med[b_], 4) for a_, b_ in PAIRS},
               "record_counted_every_step": bool((counted == steps[VARIANTS[3]]).all()), "final_state_finite": bool(torch.isfinite(sim.cur).all())}
        print(json.dumps(row), flush=True)
        results.append(row)
        sim.close()
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa-only", action="store_true", help="count instructions only (no GPU)")
    ap.add_argument("--asm", default=None, help="a hipcc -S listing of csrc/hydro_kernels.hip to read instead of compiling one")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    data["expectation"] = EXPECTATION
    if args.isa_only:
        data["isa"] = isa(args.asm)
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_statistics.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["step_loop"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"one sim per size, explicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the same initial state and step count 0 with the records reset, ending in a stream synchronise; "
                            f"variants alternate within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
