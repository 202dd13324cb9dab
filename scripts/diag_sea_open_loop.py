#!/usr/bin/env python3
"""What moving water costs in the open-loop steps: hydro_step_wrench_tiled_sea and hydro_step_wrench_aos_sea with no sea, a
current only and 1, 4 and 8 regular wave components, against their parents hydro_step_wrench_tiled and hydro_step_wrench_aos
measured in the same run.

  python scripts/diag_sea_open_loop.py              (GPU)  1 048 576 and 4 194 304 bodies -> profiles/sea_open_loop.json
  python scripts/diag_sea_open_loop.py --isa-only   (no GPU) registers, scratch and LDS of the 24 new instantiations and the
                                                          VALU / transcendental instructions of a sea kernel against its
                                                          parent (all eight component slots: the count for 8 components)

Variants: parent (the parent entry), sea_none (the _sea entry, no sea set: the parent's launch), sea_w0 (current only), sea_w1 /
sea_w4 / sea_w8 (the current plus 1 / 4 / 8 components; the seas of scripts/diag_sea.py).
Protocol: C2 buoys; the tiled entry rotates over 4 sets of (state, prev, wrench) buffers with caller-owned previous velocity,
the array-of-structs entry over 8 sets of (positions, orientations, velocities, forces, torques) - the set counts bench.py
uses for each, so that the figure is an HBM rate; every set has its own engine (parameters, engine-owned previous velocity).  A timed window is --launches back-to-back launches between two HIP
events; the variants alternate within each of --rounds rounds after one warm-up window each.  Reported: the median over the
rounds and the spread, in us per launch, and each variant over its parent."""
import argparse
import json
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "sea_open_loop.json")
SIZES = (1048576, 4194304)
VARIANTS = ("parent", "sea_none", "sea_w0", "sea_w1", "sea_w4", "sea_w8")
SETS = {"tiled": 4, "aos": 8}
DT = 1.0 / 60.0
# (new kernel, its parent, the <f32, caller's prev / -, temporal, Numba> instantiation of each)
PAIRS = {"tiled": ("wrench_tiled_sea_kernelILb0ELb0ELb0ELb0E", "wrench_tiled_kernelILi256ELb0ELb0ELb0ELb0ELb0E"),
         "aos": ("wrench_aos_sea_kernelILb0ELb0ELb0E", "wrench_aos_direct_kernelILb0ELb0ELb0E")}


def isa(asm_path=None) -> dict:
    """Whole-kernel static counts: the text from the kernel's label to its end marker (s_endpgm sits in the middle of these
    kernels), all eight component slots behind their scalar branches included."""
    from scripts import isa_mix
    asm = open(asm_path).read() if asm_path else isa_mix.assembly()
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}
    out = {"per_instantiation": {}, "against_parent": {}}
    for kernel, flags in (("wrench_tiled_sea_kernel", ("HALF", "ENGINE_PREV", "NT", "WARP")), ("wrench_aos_sea_kernel", ("HALF", "NT", "WARP"))):
        rows = {}
        for name, d in desc.items():
            if kernel not in name:
                continue
            bits = re.search(kernel + "I" + "Lb(\\d)E" * len(flags), name).groups()
            rows["<" + ", ".join(f"{k}={v}" for k, v in zip(flags, bits)) + ">"] = {
                "vgprs": int(d["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
                "scratch_bytes": int(d["private_segment_fixed_size"]), "lds_bytes": int(d["group_segment_fixed_size"])}
        out["per_instantiation"][kernel] = dict(sorted(rows.items()))
    for entry, names in PAIRS.items():
        row = {}
        for which, needle in zip(("sea", "parent"), names):
            body = re.search(r"^(_Z\S*" + needle + r"[^\s:]*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M).group(2)
            ops = re.findall(r"^\s+([a-z][a-z0-9_]+)", body, re.M)
            row[which] = {"valu": sum(isa_mix.classify(op) != "not-valu" for op in ops),
                          "fp64": sum(isa_mix.classify(op) == "fp64 arithmetic" for op in ops),
                          "transcendental": sum(isa_mix.classify(op) == "transcendental" for op in ops),
                          "scalar_loads": sum(op.startswith("s_load") for op in ops),
                          "global_loads": sum(op.startswith("global_load") for op in ops),
                          "global_stores": sum(op.startswith("global_store") for op in ops)}
        row["sea_valu_8_components"] = row["sea"]["valu"] - row["parent"]["valu"]
        row["sea_transcendental_8_components"] = row["sea"]["transcendental"] - row["parent"]["transcendental"]
        out["against_parent"][entry] = row
    return out


def measure(launches: int, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from scripts.diag_sea import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.engine import HydroEngine
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    dev = "cuda:0"
    seas = {"sea_w0": sea_of(0), "sea_w1": sea_of(1), "sea_w4": sea_of(4), "sea_w8": sea_of(8)}
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        engines = []                                                                      # one per set: parameters and the engine's previous velocity rotate too
        for _ in range(max(SETS.values())):
            engines.append(HydroEngine(n, dev, sc.rho, sc.g))
            engines[-1].set_params(sc.params, "f16")
        eng = engines[0]
        state = torch.from_numpy(scenes.to_tiled(sc.state)).to(dev)
        prev = torch.from_numpy(scenes.to_tiled(sc.prev)).to(dev)
        rows = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sc.state[:, 0:3], sc.state[:, [6, 3, 4, 5]], sc.state[:, 7:13])]
        tiled_sets = [(torch.roll(state, r * 97, 0), torch.roll(prev, r * 97, 0), eng.alloc_tiled(6, n)) for r in range(SETS["tiled"])]
        aos_sets = [tuple(torch.roll(x, r * 97 * 64, 0) for x in rows) + (torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev))
                    for r in range(SETS["aos"])]
        current = {"sea": "unset"}

        def select(v):
            want = seas.get(v)
            if current["sea"] is not want:
                torch.cuda.synchronize()
                for e in engines:
                    e.set_sea(want)
                current["sea"] = want

        def window(entry, v):
            select(v)
            t = 0.25                                                                       # a time that is no multiple of dt
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for k in range(launches):
                if entry == "tiled":
                    r = k % len(tiled_sets)
                    s, p, o = tiled_sets[r]
                    if v == "parent":
                        engines[r].step_wrench_tiled(s, n, DT, out=o, prev=p)
                    else:
                        engines[r].step_wrench_tiled_sea(s, n, DT, t, out=o, prev=p)
                else:
                    r = k % len(aos_sets)
                    p, q, vel, f, tq = aos_sets[r]
                    if v == "parent":
                        engines[r].step_wrench_aos(p, q, vel, DT, f, tq)
                    else:
                        engines[r].step_wrench_aos_sea(p, q, vel, DT, t, f, tq)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) * 1e3 / launches                               # us per launch

        for entry in ("tiled", "aos"):
            for v in VARIANTS:
                window(entry, v)                                                           # warm-up, discarded
            times = {v: [] for v in VARIANTS}
            for _ in range(rounds):
                for v in VARIANTS:
                    times[v].append(window(entry, v))
            med = {v: statistics.median(t) for v, t in times.items()}
            row = {"entry": entry, "bodies": n, "coefficients": "f16", "sets": SETS[entry], "launches_per_window": launches, "rounds": rounds,
                   "us_per_launch": {v: {"median": round(med[v], 3), "min": round(min(t), 3), "max": round(max(t), 3)} for v, t in times.items()},
                   "over_parent": {v: round(med[v] / med["parent"], 4) for v in VARIANTS if v != "parent"},
                   "us_over_parent": {v: round(med[v] - med["parent"], 3) for v in VARIANTS if v != "parent"}}
            print(json.dumps(row), flush=True)
            results.append(row)
        for e in engines:
            e.close()
        del tiled_sets, aos_sets, state, prev, rows
        torch.cuda.empty_cache()
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa-only", action="store_true", help="read the assembly only (no GPU)")
    ap.add_argument("--asm", default=None, help="with --isa-only: an existing `hipcc -S` output of the library instead of compiling one")
    ap.add_argument("--launches", type=int, default=200, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.isa_only:
        data["isa"] = isa(args.asm)
        print(json.dumps(data["isa"]["against_parent"]))
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"C2 buoys, fp16 coefficients; tiled entry over {SETS['tiled']} rotating sets with caller-owned previous velocity, "
                            f"array-of-structs entry over {SETS['aos']}; windows of {args.launches} back-to-back launches between two HIP events; "
                            f"variants alternate within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.launches, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
