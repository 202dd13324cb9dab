#!/usr/bin/env python3
"""What an irregular or a finite-depth sea costs in the open-loop steps: hydro_step_wrench_tiled_irr and hydro_step_wrench_aos_irr
with no sea, an 8-wave sea, a current-only spectrum and 8, 16 and 64 components in deep water and at h = 20 m, against the parent
entries and the _sea entries with 8 waves measured in the same run - the parent commit's kernels, byte for byte (DESIGN.md
section 33: scripts/asm_symbols.py), never the code under test.

  python scripts/diag_sea_spectrum_open_loop.py              (GPU)  1 048 576 and 4 194 304 bodies -> profiles/sea_spectrum_open_loop.json
  python scripts/diag_sea_spectrum_open_loop.py --isa-only   (no GPU) registers, scratch and LDS of the 48 new instantiations, and the
                                                                  VALU / transcendental instructions per component of a trip of the
                                                                  component loops against the _sea kernels' (whole kernel over 8 slots)

Variants: parent; sea_w8 (the _sea entry, 8 waves); irr_none (the _irr entry, nothing set: the parent's launch); irr_sea8 (the
_irr entry over the 8-wave sea: the _sea launch); irr_w0 (a current-only spectrum); irr_w8 / irr_w16 / irr_w64 (JONSWAP, deep);
fd_w8 / fd_w16 / fd_w64 (the same at h = 20 m).
Protocol: that of scripts/diag_sea_open_loop.py - C2 buoys, fp16 coefficients; the tiled entry rotates over 4 sets of (state, prev,
wrench) buffers with caller-owned previous velocity, the array-of-structs entry over 8 sets, every set with its own engine; a timed
window is --launches back-to-back launches between two HIP events; the variants alternate within each of --rounds rounds after one
warm-up window each, and each round starts two variants further on (a first run in ONE fixed order left the parent, always behind
the heaviest variant, 11 - 16 % slower than the same launch behind a light one: DESIGN.md section 33).  Reported: the median over the
rounds and the spread, in us per launch, each variant over the parent."""
import argparse
import json
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "sea_spectrum_open_loop.json")
SIZES = (1048576, 4194304)
VARIANTS = ("parent", "sea_w8", "irr_none", "irr_sea8", "irr_w0", "irr_w8", "irr_w16", "irr_w64", "fd_w8", "fd_w16", "fd_w64")
SETS = {"tiled": 4, "aos": 8}
DT = 1.0 / 60.0
DEPTH = 20.0
ROTATE = 2        # with 11 variants and 5 rounds every variant follows five different predecessors; the parent never follows fd_w64 twice

# Written BEFORE the first run, from figures the project already had:
#   a component of the 8-wave sea costs 0.67 us (tiled) and 0.47 us (array-of-structs) per launch at 1 M bodies,
#                         with ~29 VALU instructions per component; a current alone 8 % (tiled: p_x and p_y are loaded) and 1.6 %
#   sections 29 and 32  : spectrum_water issues 37 VALU per component and body, depth_water 42 (two passes, nothing kept)
#   section 32          : the RESIDENT step with 64 components takes 76.9 us (deep) and 85.8 us (h = 20 m) at 1 M bodies - wrench,
#                         integrator and the state's round trip included, so an upper bound on what 64 components add here
# Scaling section 23's slope by the instruction ratio: 0.67 * 37 / 29 = 0.85 us and 0.67 * 42 / 29 = 0.97 us per component (tiled),
# 0.47 * 37 / 29 = 0.60 us and 0.68 us (array-of-structs), at 1 M bodies; four times that at 4 M.  The parent is memory-bound and the
# components are arithmetic, so part of the first components hides behind the loads: the ranges reach down to 0.7 of the slope.
EXPECTATION = {
    "us_per_component_at_1M": {"tiled": {"deep": [0.60, 0.85], "h20": [0.68, 0.97]}, "aos": {"deep": [0.42, 0.60], "h20": [0.48, 0.68]}},
    "us_over_parent_at_1M": {"tiled": {"irr_w8": [4.8, 6.8], "irr_w16": [9.5, 13.6], "irr_w64": [38.0, 54.5], "fd_w8": [5.4, 7.8], "fd_w16": [10.9, 15.5],
                                       "fd_w64": [43.5, 62.0]},
                             "aos": {"irr_w8": [3.4, 4.8], "irr_w16": [6.7, 9.6], "irr_w64": [26.9, 38.4], "fd_w8": [3.8, 5.4], "fd_w16": [7.6, 10.9],
                                     "fd_w64": [30.5, 43.6]}},
    "fd_over_deep_at_64": [1.08, 1.14],          # (42 / 37 = 1.135 on the components alone; section 32 measured 1.115 resident)
    "irr_w0_over_parent": {"tiled": [1.00, 1.10], "aos": [1.00, 1.04]},
    "identities": "irr_none is the parent's launch and irr_sea8 the _sea launch: both within the parent's own spread in the session",
    "upper_bound_64_components_at_1M_us": {"deep": 76.9, "h20": 85.8},
}
# (new kernel, the _sea kernel, its parent: the <f32, caller's prev / -, temporal, Numba> instantiation of each)
TRIO = {"tiled": ("wrench_tiled_irr_kernelILb0ELb0ELb0ELb0ELb{d}E", "wrench_tiled_sea_kernelILb0ELb0ELb0ELb0E", "wrench_tiled_kernelILi256ELb0ELb0ELb0ELb0ELb0E"),
        "aos": ("wrench_aos_irr_kernelILb0ELb0ELb0ELb{d}E", "wrench_aos_sea_kernelILb0ELb0ELb0E", "wrench_aos_direct_kernelILb0ELb0ELb0E")}


def _loops(body):
    """The loops of a function's text - the lines from a label to a branch back to it - as lists of opcodes."""
    lines = body.splitlines()
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i + 1) <= i:
            out.append([re.match(r"\s+([a-z][a-z0-9_]+)", x).group(1) for x in lines[labels[m.group(1)]:i + 1] if re.match(r"\s+[a-z]", x)])
    return out


def isa(asm_path=None) -> dict:
    from scripts import isa_mix
    asm = open(asm_path).read() if asm_path else isa_mix.assembly()
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}
    body = lambda needle: re.search(r"^(_Z\S*" + needle + r"[^\s:]*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M).group(2)  # noqa: E731
    count = lambda ops: {"valu": sum(isa_mix.classify(op) != "not-valu" for op in ops),  # noqa: E731
                         "fp64": sum(isa_mix.classify(op) == "fp64 arithmetic" for op in ops),
                         "transcendental": sum(isa_mix.classify(op) == "transcendental" for op in ops),
                         "scalar_loads": sum(op.startswith("s_load") for op in ops),
                         "vector_memory_or_lds": sum(op.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")) for op in ops)}
    out = {"per_instantiation": {}, "per_component": {}}
    for kernel, flags in (("wrench_tiled_irr_kernel", ("HALF", "ENGINE_PREV", "NT", "WARP", "DEPTH")), ("wrench_aos_irr_kernel", ("HALF", "NT", "WARP", "DEPTH"))):
        rows = {}
        for name, d in desc.items():
            if kernel not in name:
                continue
            bits = re.search(kernel + "I" + "Lb(\\d)E" * len(flags), name).groups()
            rows["<" + ", ".join(f"{k}={v}" for k, v in zip(flags, bits)) + ">"] = {
                "vgprs": int(d["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
                "scratch_bytes": int(d["private_segment_fixed_size"]), "lds_bytes": int(d["group_segment_fixed_size"])}
        out["per_instantiation"][kernel] = dict(sorted(rows.items()))
    for entry, (irr, sea, parent) in TRIO.items():
        ops = lambda needle: re.findall(r"^\s+([a-z][a-z0-9_]+)", body(needle), re.M)  # noqa: E731
        sea_ops, parent_ops = count(ops(sea)), count(ops(parent))
        row = {"sea_kernel_per_component_of_8": {k: round((sea_ops[k] - parent_ops[k]) / 8.0, 2) for k in ("valu", "fp64", "transcendental")}}
        for depth in (0, 1):
            loops = [count(l) for l in _loops(body(irr.format(d=depth)))]
            assert len(loops) == 4, (entry, depth, len(loops))
            # the loops in program order: first pass by four, its remainder, second pass by four, its remainder
            row["deep" if depth == 0 else "finite_depth"] = {
                "first_pass_group_of_four": loops[0], "first_pass_remainder_trip": loops[1], "second_pass_group_of_four": loops[2],
                "second_pass_remainder_trip": loops[3],
                "per_component_in_a_group": {k: round((loops[0][k] + loops[2][k]) / 4.0, 2) for k in ("valu", "fp64", "transcendental", "scalar_loads")},
                "per_component_in_the_remainder": {k: loops[1][k] + loops[3][k] for k in ("valu", "fp64", "transcendental", "scalar_loads")}}
        out["per_component"][entry] = row
    return out


def measure(launches: int, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from scripts.diag_sea import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.engine import HydroEngine
    from silver2_isaacsim_amd.sea import SeaSpectrum, jonswap
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    dev = "cuda:0"
    kw = dict(seed=3, spread="cos2", current=(0.3, -0.1, 0.0))
    seas = {"sea_w8": sea_of(8), "irr_sea8": sea_of(8), "irr_w0": SeaSpectrum((0.3, -0.1, 0.0))}
    for k in (8, 16, 64):
        seas[f"irr_w{k}"] = jonswap(1.5, 7.0, 25.0, components=k, **kw)
        seas[f"fd_w{k}"] = jonswap(1.5, 7.0, 25.0, components=k, depth=DEPTH, **kw)
    seas["irr_sea8"] = seas["sea_w8"]
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
            if current["sea"] is want:
                return
            torch.cuda.synchronize()
            for e in engines:
                e.set_sea(None); e.set_sea_spectrum(None); e.set_sea_finite_depth(None)
                if want is None:
                    continue
                if getattr(want, "depth", None) is not None:
                    e.set_sea_finite_depth(want, n)
                elif isinstance(want, SeaSpectrum):
                    e.set_sea_spectrum(want)
                else:
                    e.set_sea(want)
            current["sea"] = want

        def window(entry, v):
            select(v)
            t = 0.25                                                                       # a time that is no multiple of dt
            kind = "" if v == "parent" else "_sea" if v == "sea_w8" else "_irr"
            tiled, aos = (getattr(HydroEngine, "step_wrench_tiled" + kind), getattr(HydroEngine, "step_wrench_aos" + kind))
            extra = () if v == "parent" else (t,)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for k in range(launches):
                if entry == "tiled":
                    r = k % len(tiled_sets)
                    s, p, o = tiled_sets[r]
                    tiled(engines[r], s, n, DT, *extra, out=o, prev=p)
                else:
                    r = k % len(aos_sets)
                    p, q, vel, f, tq = aos_sets[r]
                    aos(engines[r], p, q, vel, DT, *extra, f, tq)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) * 1e3 / launches                               # us per launch

        for entry in ("tiled", "aos"):
            for v in VARIANTS:
                window(entry, v)                                                           # warm-up, discarded
            times = {v: [] for v in VARIANTS}
            for r in range(rounds):                                                        # round r starts ROTATE * r variants further on:
                for v in VARIANTS[ROTATE * r % len(VARIANTS):] + VARIANTS[:ROTATE * r % len(VARIANTS)]:   # no variant keeps one predecessor
                    times[v].append(window(entry, v))
            med = {v: statistics.median(t) for v, t in times.items()}
            row = {"entry": entry, "bodies": n, "coefficients": "f16", "sets": SETS[entry], "launches_per_window": launches, "rounds": rounds,
                   "us_per_launch": {v: {"median": round(med[v], 3), "min": round(min(t), 3), "max": round(max(t), 3)} for v, t in times.items()},
                   "over_parent": {v: round(med[v] / med["parent"], 4) for v in VARIANTS if v != "parent"},
                   "us_over_parent": {v: round(med[v] - med["parent"], 3) for v in VARIANTS if v != "parent"},
                   "us_per_component": {"deep": round((med["irr_w64"] - med["irr_w8"]) / 56.0, 4), "h20": round((med["fd_w64"] - med["fd_w8"]) / 56.0, 4)},
                   "fd_over_deep_at_64": round(med["fd_w64"] / med["irr_w64"], 4),
                   "irr_sea8_over_sea_w8": round(med["irr_sea8"] / med["sea_w8"], 4)}
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
    data["expectation_written_before_the_run"] = EXPECTATION
    if args.isa_only:
        data["isa"] = isa(args.asm)
        print(json.dumps(data["isa"]["per_component"]))
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"C2 buoys, fp16 coefficients; tiled entry over {SETS['tiled']} rotating sets with caller-owned previous velocity, "
                            f"array-of-structs entry over {SETS['aos']}; windows of {args.launches} back-to-back launches between two HIP events; "
                            f"variants alternate within each of {args.rounds} rounds after one warm-up window each, every round starting {ROTATE} "
                            f"variants further on; JONSWAP Hs 1.5 m, Tp 7 s, cos^2, "
                            f"finite depth h = {DEPTH:g} m; the parent and sea_w8 kernels are the parent commit's, byte for byte")
        data["measurements"] = measure(args.launches, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
