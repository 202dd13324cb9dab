#!/usr/bin/env python3
"""What a mooring spread costs in the resident closed loop: hydro_step_fused_tiled_multi_spread - up to four anchored lines per
body, each evaluated in a loop over the layers that reads its record from the caller's buffer - against the path a single
line takes (set_mooring with track_extremes: hydro_step_fused_tiled_multi_ext, whose kernels this feature leaves
byte-identical): the baseline, measured in the same run.

  python scripts/diag_mooring_spread.py              (GPU)  C2 buoys at 4 096 and 1 048 576 bodies -> profiles/mooring_spread.json
  python scripts/diag_mooring_spread.py --isa-only   (no GPU) registers, LDS and scratch of the 32 instantiations beside the
                                                            link-tension kernel's, and the instructions of the layer loop, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, all in still water with the
extremes tracked and every other option absent:
  line           one taut line per body through set_mooring: the parked line of the extremes kernel
  spread1        the same record as a spread of one layer: the line through the loop
  spread3_taut   three taut lines per body at 120 degrees
  spread3_one    the line of `line` in layer 0 and two layers of zeros: two trips that skip
Protocol (that of scripts/diag_tether.py): every timed window starts from the same initial state and step
count 0, lasts at least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate
within each of --rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max),
in us per physics step.  No ratio is gated.  The expectation written down beforehand: one layer through
the loop costs about what the parked line costs (section 24 found 1.08 - 1.19 x for the net), and an empty layer about half a
taut one."""

import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "mooring_spread.json")
CHUNK = 64
SIZES = (4096, 1048576)
VARIANTS = ("line", "spread1", "spread3_taut", "spread3_one")
PAIRS = (("spread1", "line"), ("spread3_taut", "line"), ("spread3_one", "line"), ("spread3_one", "spread1"), ("spread3_taut", "spread1"))
KERNELS = ("step_fused_multi_peak_tiled_kernel", "step_fused_multi_spread_tiled_kernel")
EXPECTATION = ("one layer through the loop costs about what the parked line costs (1.08 - 1.19 x was the net's); an empty layer costs about "
               "half a taut one")


def isa() -> dict:
    """Over the 32 instantiations of the new kernel: VGPRs, SGPRs, LDS bytes and scratch, each beside the link-tension kernel's
    instantiation of the same flags (the spread parks nothing: its LDS is that kernel's less the line's nine slots per lane,
    9 216 bytes).  And of the <f32, temporal, no KE, Numba> instantiations, per drag form: the instructions of the MOORING LAYER
    LOOP - the depth-2 loop inside the step loop that holds no ds_bpermute_b32 (the others are the net's) - its whole body,
    the evaluation behind the ballot included."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    count = lambda loop: {"instructions": len(loop), "valu": sum(isa_mix.classify(op) != "not-valu" for op in loop),  # noqa: E731
                          "global_load_dword": sum(op == "global_load_dword" for op in loop),
                          "ds_read": sum(op.startswith("ds_read") for op in loop), "ds_bpermute_b32": sum(op == "ds_bpermute_b32" for op in loop),
                          "global_store_or_atomic": sum(op.startswith(("global_store", "global_atomic")) for op in loop),
                          "scratch": sum(op.startswith("scratch_") for op in loop)}
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        body = re.search(r"^(_Z\S*" + KERNELS[1] + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
        blocks = re.split(r"^(\.LBB\d+_\d+:[^\n]*(?:\n\s*;[^\n]*)*)\n", body, flags=re.M)               # a label with the comment lines that follow it
        loops = {}
        for label, text in zip(blocks[1::2], blocks[2::2]):
            if "Depth=2" not in label:
                continue
            own = re.match(r"\.L(BB\d+_\d+):", label).group(1)
            inside = re.search(r"Header=(BB\d+_\d+) Depth=2", label)
            loops.setdefault(inside.group(1) if inside else own, []).append(text)
        layer_loops = [count(ops("\n".join(texts))) for texts in loops.values()]
        mooring = [c for c in layer_loops if c["ds_bpermute_b32"] == 0 and c["global_load_dword"] > 0]
        out["loop"][drag] = {"depth_2_loops": len(layer_loops), "mooring_layer_loop": mooring[0] if len(mooring) == 1 else mooring,
                             "rolled": len(mooring) == 1 and mooring[0]["global_load_dword"] == 9}
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if any(k in m.group(1) for k in KERNELS)}
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    peak_of = {flags_of(k): d for k, d in desc.items() if KERNELS[0] in k}
    spread = {k: d for k, d in desc.items() if KERNELS[1] in k}
    span = lambda key: [min(int(d[key]) for d in spread.values()), max(int(d[key]) for d in spread.values())]  # noqa: E731
    out["instantiations"] = {"count": len(spread), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    per = {}
    for name, d in spread.items():
        peak = peak_of[flags_of(name)]
        vgprs = int(d["next_free_vgpr"])
        per["<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags_of(name))) + ">"] = {
            "vgprs": vgprs, "peak_kernel_vgprs": int(peak["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]), "peak_kernel_sgprs": int(peak["next_free_sgpr"]),
            "waves_per_simd": 512 // (-(-vgprs // 8) * 8), "lds_bytes": int(d["group_segment_fixed_size"]),
            "peak_kernel_lds_bytes": int(peak["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
    out["per_instantiation"] = dict(sorted(per.items()))
    out["conditions_met"] = all(v["scratch_bytes"] == 0 and v["vgprs"] <= 168 and v["waves_per_simd"] >= 3 and v["lds_bytes"] <= v["peak_kernel_lds_bytes"]
                                for v in per.values()) and len(per) == 32 and all(r["rolled"] for r in out["loop"].values())
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import MooringSpread
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        assert n % 64 == 0
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10].astype(np.float64)
        pos = sc.state[:, 0:3].astype(np.float64)
        k, c = MooringSpread.for_body(mass, sc.dt, 3)
        phi = 2.0 * np.pi * np.arange(3) / 3.0
        anchors = np.stack([pos[:, None, 0] + 6.0 * np.cos(phi)[None, :], pos[:, None, 1] + 6.0 * np.sin(phi)[None, :],
                            np.broadcast_to(pos[:, None, 2] - 8.0, (n, 3))], axis=2)                # reach 10 m; 9.9 m of line: taut
        three = dict(anchors=anchors, length=9.9, stiffness=np.repeat(k[:, None], 3, axis=1), damping=np.repeat(c[:, None], 3, axis=1))
        one = dict(anchor=anchors[:, 0], length=9.9, stiffness=k, damping=c)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        sim.track_extremes()
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.synchronize()
            sim.clear_mooring()
            sim.clear_mooring_spread()
            if v == "line":
                sim.set_mooring(**one)
            elif v == "spread1":
                sim.set_mooring_spread(anchors[:, :1], length=9.9, stiffness=k[:, None], damping=c[:, None])
            else:
                sim.set_mooring_spread(**three)
                if v == "spread3_one":
                    with torch.cuda.stream(sim.stream):
                        sim.mooring_spread[:, 9:27].zero_()                                   # layers 1 and 2: nobody has a line

        def window(v, steps):
            select(v)
            with torch.cuda.stream(sim.stream):
                sim.cur.copy_(start[0]); sim.old.copy_(start[1])
            sim.steps_done = 0
            sim.extremes.reset()
            sim.synchronize()
            t0 = time.perf_counter()
            sim.run_resident(steps, chunk=CHUNK)
            sim.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6                                  # us per physics step

        steps, loaded = {}, {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                              # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                               # warm-up, discarded
            loaded[v] = float((sim.extremes.tension_max() > 0.0).mean())                      # share of the bodies whose lines carried load
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "implicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "ratios": {f"{a_}_over_{b_}": round(med[a_] / med[b_], 4) for a_, b_ in PAIRS},
               "share_of_bodies_whose_lines_carried_load": loaded, "final_state_finite": bool(torch.isfinite(sim.cur).all())}
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
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_mooring_spread.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["loop"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["expectation"] = EXPECTATION
        data["protocol"] = (f"one sim per size, implicit drag, still water, extremes tracked, run_resident(chunk={CHUNK}), the variant switched between "
                            f"windows; windows of >= {args.window} s from the same initial state and step count 0, ending in a stream synchronise; "
                            f"variants alternate within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
