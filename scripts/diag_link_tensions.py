#!/usr/bin/env python3
"""What tracking the peak tension of every tether link costs in the resident closed loop: hydro_step_fused_tiled_multi_peak -
the net kernel with one no-return integer maximum behind the wrench of every line that pulls - against
hydro_step_fused_tiled_multi_net, whose kernels this feature leaves byte-identical: the baseline, measured in the same run.

  python scripts/diag_link_tensions.py              (GPU)  C2 buoys at 4 096 and 1 048 576 bodies -> profiles/link_tensions.json
  python scripts/diag_link_tensions.py --isa-only   (no GPU) registers, LDS and scratch of the 32 instantiations beside the net
                                                           kernel's, and the instructions of the layer loop's body, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, all in still water with
every other option absent (the nets are those of scripts/diag_tether_net.py):
  net2_none     a net of two layers of zeros through the net entry: nobody tethered, every wave skips twice
  peak2_none    the same net with track_link_tensions(): the new entry, no line, no update
  net2_chain    every tile of 64 one chain 0 - 1 - ... - 63 through the net entry: two layers
  peak2_chain   the same chain with track_link_tensions(): one update per pulling line and step
(in still water tied bodies draw together within a window and lines end slack: the share that still pulls at the end of a
window is reported; only a pulling line updates its slot).
Protocol (that of scripts/diag_tether.py): every timed window starts from the same initial state and step count 0, lasts at
least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per
physics step.  No ratio is gated.  The expectation written down beforehand: empty layers cost nothing extra, and a taut layer
costs at most one more round trip to L2 per step."""

import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "link_tensions.json")
CHUNK = 64
SIZES = (4096, 1048576)
VARIANTS = ("net2_none", "peak2_none", "net2_chain", "peak2_chain")
PAIRS = (("peak2_none", "net2_none"), ("peak2_chain", "net2_chain"))
KERNELS = ("step_fused_multi_net_tiled_kernel", "step_fused_multi_peak_tiled_kernel")


def isa() -> dict:
    """Over the 32 instantiations of the new kernel: VGPRs, SGPRs, LDS bytes and scratch, each beside the net kernel's
    instantiation of the same flags (the policy allocates no LDS: the bytes must be equal).  And of the <f32, temporal, no KE,
    Numba> instantiations, per drag form: the instructions of the LAYER LOOP (the depth-2 loop inside the step loop) - its
    whole body, the evaluation behind the ballot included - and of the step loop around it, beside the net kernel's."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    count = lambda loop: {"instructions": len(loop), "valu": sum(isa_mix.classify(op) != "not-valu" for op in loop),  # noqa: E731
                          "ds_bpermute_b32": sum(op == "ds_bpermute_b32" for op in loop),
                          "global_load_dword": sum(op == "global_load_dword" for op in loop),
                          "global_atomic_umax": sum(op == "global_atomic_umax" for op in loop),
                          "global_store": sum(op.startswith("global_store") for op in loop),
                          "other_atomics": sum("atomic" in op and op != "global_atomic_umax" for op in loop)}
    out = {"loop": {}}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        row = {}
        for name in KERNELS:
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            blocks = re.split(r"^(\.LBB\d+_\d+:[^\n]*(?:\n\s*;[^\n]*)*)\n", body, flags=re.M)           # a label with the comment lines that follow it
            labelled = list(zip(blocks[1::2], blocks[2::2]))
            row[name] = {"step_loop": count(ops("\n".join(text for label, text in labelled if "Loop" in label))),
                         "layer_loop": count(ops("\n".join(text for label, text in labelled if "Depth=2" in label)))}
            if name == KERNELS[1]:
                atomics = [l.strip() for l in body.splitlines() if l.strip().startswith("global_atomic_umax")]
                # no-return: an address (a VGPR pair, or a VGPR offset on an SGPR base) and ONE data register, no destination, no sc0
                row["update"] = {"instructions": atomics,
                                 "no_return": all(re.fullmatch(r"global_atomic_umax (v\[\d+:\d+\], v\d+, off|v\d+, v\d+, s\[\d+:\d+\])( offset:\d+)?", a)
                                                  for a in atomics)}
        row["unrolled"] = row[KERNELS[1]]["step_loop"]["ds_bpermute_b32"] != 6                        # six exchanges in the whole kernel: one evaluation
        out["loop"][drag] = row
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if any(k in m.group(1) for k in KERNELS)}
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    net_of = {flags_of(k): d for k, d in desc.items() if KERNELS[0] in k}
    peak = {k: d for k, d in desc.items() if KERNELS[1] in k}
    span = lambda key: [min(int(d[key]) for d in peak.values()), max(int(d[key]) for d in peak.values())]  # noqa: E731
    out["instantiations"] = {"count": len(peak), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    per = {}
    for name, d in peak.items():
        net = net_of[flags_of(name)]
        vgprs = int(d["next_free_vgpr"])
        per["<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags_of(name))) + ">"] = {
            "vgprs": vgprs, "net_kernel_vgprs": int(net["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]), "net_kernel_sgprs": int(net["next_free_sgpr"]),
            "waves_per_simd": 512 // (-(-vgprs // 8) * 8), "lds_bytes": int(d["group_segment_fixed_size"]),
            "net_kernel_lds_bytes": int(net["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
    out["per_instantiation"] = dict(sorted(per.items()))
    out["conditions_met"] = all(v["scratch_bytes"] == 0 and v["vgprs"] <= 168 and v["waves_per_simd"] >= 3 and v["lds_bytes"] == v["net_kernel_lds_bytes"]
                                for v in per.values()) and len(per) == 32 and not any(r["unrolled"] for r in out["loop"].values()) \
        and all(r["update"]["no_return"] and len(r["update"]["instructions"]) == 1 for r in out["loop"].values())
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import DEFAULT_C, DEFAULT_K
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        assert n % 64 == 0
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10].astype(np.float64)
        pos = sc.state[:, 0:3].astype(np.float64)
        # a chain through every tile: link i joins bodies i and i + 1 unless i is a tile's last lane; layers alternate along the tile
        i = np.arange(n - 1)
        i = i[i % 64 != 63]
        chain = np.stack([i, i + 1], axis=1)
        lighter = np.minimum(mass[i], mass[i + 1])
        ck, cc = DEFAULT_K * lighter / (4.0 * sc.dt ** 2), DEFAULT_C * lighter / (4.0 * sc.dt)        # two such lines at a body: a tenth, a half of the rule
        spans = np.linalg.norm(pos[i + 1] - pos[i], axis=1)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.synchronize()
            sim.clear_link_tensions()
            sim.set_tether_net(chain, length=0.5 * spans, stiffness=ck, damping=cc, layer=i % 2)
            assert sim.tether_layers == 2
            if v.endswith("_none"):
                with torch.cuda.stream(sim.stream):
                    sim.tether_net.zero_()                                                # two layers in which nobody has a line
            if v.startswith("peak"):
                sim.track_link_tensions()

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

        steps, pulling, peaks = {}, {}, {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                          # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                           # warm-up, discarded
            layers, _ = sim.engine.tether_net_wrench(sim.cur, sim.tether_net, n, sim.tether_layers)
            pulling[v] = float(np.any([scenes.from_tiled(w.cpu().numpy(), n).any(axis=1) for w in layers], axis=0).mean())
            if sim.link_tensions is not None:
                peaks[v] = float((sim.link_tensions.record() > 0.0).any(axis=1).mean())   # share of the bodies with a peak on record
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "implicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "ratios": {f"{a_}_over_{b_}": round(med[a_] / med[b_], 4) for a_, b_ in PAIRS},
               "share_pulling_at_the_end_of_a_window": pulling, "share_with_a_peak_on_record": peaks,
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
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_link_tensions.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["loop"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["expectation"] = "empty layers cost nothing extra; a taut layer costs at most one more round trip to L2 per step"
        data["protocol"] = (f"one sim per size, implicit drag, still water, run_resident(chunk={CHUNK}), the variant switched between windows; windows of "
                            f">= {args.window} s from the same initial state and step count 0, ending in a stream synchronise; variants alternate "
                            f"within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
