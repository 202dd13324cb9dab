#!/usr/bin/env python3
"""What a finite-depth sea costs in the resident closed loop: hydro_step_fused_tiled_multi_fd - depth_water, the second exponential
and the clamp at the bed in every component of the second pass - against the kernels this feature leaves byte-identical (the _ens
and _ens_stat kernels under a one-member set_sea_ensemble), measured in the same run.

  python scripts/diag_sea_depth.py              (GPU)  C2 buoys, 64 components -> profiles/sea_depth.json
  python scripts/diag_sea_depth.py --isa-only   (no GPU) registers, LDS and scratch of the 64 instantiations beside the _ens kernels they
                                                       are built on, and the instructions of every component loop, from hipcc -S
                                                       (--asm FILE: a listing at hand)

Two configurations, explicit drag: "bare" (nothing but the sea: the _ens / _fd kernels) and "design" (a three-line spread, the
extremes and track_statistics(("z", "tension")): the _ens_stat / _fd_stat kernels - a design-load study).
Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, at 4 096 and 1 048 576 bodies:
  ens   set_sea(SeaEnsemble of ONE member that covers n): a JONSWAP sea of 64 deep-water components - the parent's kernels
  fd    set_sea(the same bins at depth 20 m: jonswap(..., depth=20)) as one member that covers n - the new kernels
Protocol (that of scripts/diag_sea_spectrum.py): every timed window starts from the same initial state and
step count 0 with the records reset, lasts at least --window seconds of back-to-back launches of run_resident(chunk=64) and ends in
a stream synchronise; the variants alternate within each of --rounds rounds, after a warm-up window each.  Reported: the median
over the rounds and the range, in us per physics step.  No ratio is gated.  The expectation written down beforehand is EXPECTATION
(DESIGN.md section 32)."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "sea_depth.json")
CHUNK = 64
SIZES = (4096, 1048576)
DEPTH = 20.0
CONFIGS = ("bare", "design")
VARIANTS = ("ens", "fd")
FAMILIES = {"step_fused_multi_fd_tiled_kernel": "step_fused_multi_ens_tiled_kernel",
            "step_fused_multi_fd_stat_tiled_kernel": "step_fused_multi_ens_stat_tiled_kernel"}
EXPECTATION = ("from the code, before any measurement: depth_water adds to each component of the second pass one v_exp_f32, the fma that forms "
               "its argument, an add, a subtract - and the clamp, one v_max_f32 per body and step, outside the loops; gl_j rides in the record's "
               "pad word, which the group's scalar loads already fetch, and -h is one more kernel argument.  So one transcendental and about four "
               "VALU join the 37 VALU instructions of a component (section 29: 15 + 22 in the two passes, 4 of them transcendental), 42 for 37.  "
               "A step without a sea is about 530 VALU instructions, so where the loop is bound by VALU issue a bare step of 64 components should "
               "cost (530 + 64 * 42) / (530 + 64 * 37) = 1.11 times the deep one by instruction count; section 29 measured the deep loop 1.18 times "
               "dearer than its count (4.0 for 3.4), which points at the transcendentals' quarter rate - pricing each at four issue slots gives "
               "(530 + 64 * 57) / (530 + 64 * 49) = 1.14.  Expected: 1.11 to 1.14 for the bare step at 1 048 576 bodies; somewhat less with the "
               "design configuration, whose spread, extremes and statistics add work the depth does not touch (1.09 to 1.13); and no more than "
               "that at 4 096 bodies, where 64 tiles leave three quarters of the CUs idle and a step is latency, not issue.  Registers: the "
               "second exponential is live only inside a component, so the kernels should stay within a few VGPRs of the _ens kernels', at "
               "3 waves per SIMD, without scratch; SGPRs at the 100 they stand at")


def isa(asm_path=None) -> dict:
    """Over the 2 x 32 instantiations: VGPRs, SGPRs, LDS bytes and scratch beside the _ens instantiation of the same flags; and of EVERY
    instantiation the component loops - the depth-2 loops inside the step loop that hold a v_cos_f32 - with their memory instructions by
    kind (scalar loads only) and their exponentials per component (one in the first-pass loops' absence of any, two in the second pass)."""
    from scripts import isa_mix
    asm = open(asm_path).read() if asm_path else isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M)}

    def component_loops(name):
        body, loops = bodies[name], []
        for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(?:\s*;[^\n]*\n)*", body, re.M):      # a label with the comment lines that follow it
            if "Loop Header: Depth=2" not in m.group(0):
                continue
            back = [b.end() for b in re.finditer(r"^\s+s_c?branch\S* " + re.escape(m.group(1)) + r"$", body, re.M)]
            loop = ops(body[m.start():max(back)]) if back else []
            if not any(op.startswith("v_cos_f32") for op in loop):
                continue
            sines = sum(op.startswith("v_sin_f32") for op in loop)
            loops.append({"components_per_trip": sum(op.startswith("v_cos_f32") for op in loop), "second_pass": sines > 0, "instructions": len(loop),
                          "valu": sum(op.startswith("v_") for op in loop), "exponentials": sum(op.startswith("v_exp_f32") for op in loop),
                          "scalar_loads": sum(op.startswith("s_load") or op.startswith("s_buffer_load") for op in loop),
                          "lds": sum(op.startswith("ds_") for op in loop),
                          "vector_memory": sum(op.startswith(("global_", "flat_", "buffer_", "scratch_")) for op in loop)})
        return loops

    def per_component(loops):
        """VALU instructions per component of the two passes together, from the groups-of-four loops."""
        groups = [l for l in loops if l["components_per_trip"] == 4]
        return sum(l["valu"] for l in groups) / 4.0 if len(groups) == 2 else None

    per, ok = {}, True
    for new, base in FAMILIES.items():
        mine = {flags_of(k): (k, d) for k, d in desc.items() if re.search(r"\d" + new + "I", k)}
        theirs = {flags_of(k): (k, d) for k, d in desc.items() if re.search(r"\d" + base + "I", k)}
        ok = ok and len(mine) == 32
        for flags, (name, d) in sorted(mine.items()):
            vgprs, loops = int(d["next_free_vgpr"]), component_loops(name)
            base_name, base_d = theirs[flags]
            second = [l for l in loops if l["second_pass"]]
            row = {"vgprs": vgprs, "built_on_vgprs": int(base_d["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
                   "built_on_sgprs": int(base_d["next_free_sgpr"]), "waves_per_simd": 512 // (-(-vgprs // 8) * 8),
                   "lds_bytes": int(d["group_segment_fixed_size"]), "built_on_lds_bytes": int(base_d["group_segment_fixed_size"]),
                   "scratch_bytes": int(d["private_segment_fixed_size"]), "component_loops": len(loops),
                   "second_pass_exponentials_per_component": sorted({l["exponentials"] / l["components_per_trip"] for l in second}),
                   "valu_per_component": per_component(loops), "built_on_valu_per_component": per_component(component_loops(base_name)),
                   "component_loop_scalar_loads": sum(l["scalar_loads"] for l in loops), "component_loop_lds": sum(l["lds"] for l in loops),
                   "component_loop_vector_memory": sum(l["vector_memory"] for l in loops)}
            ok = ok and (row["scratch_bytes"] == 0 and vgprs <= 168 and row["waves_per_simd"] >= 3 and row["lds_bytes"] == row["built_on_lds_bytes"]
                         and len(loops) == 4 and row["component_loop_scalar_loads"] > 0 and row["component_loop_lds"] == 0
                         and row["component_loop_vector_memory"] == 0 and row["second_pass_exponentials_per_component"] == [2.0])
            per[new + "<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags)) + ">"] = row
    span = lambda key: [min(v[key] for v in per.values()), max(v[key] for v in per.values())]  # noqa: E731
    out = {"instantiations": {"count": len(per), "vgprs": span("vgprs"), "built_on_vgprs": span("built_on_vgprs"), "sgprs": span("sgprs"),
                              "built_on_sgprs": span("built_on_sgprs"), "lds_bytes": span("lds_bytes"), "scratch_bytes": span("scratch_bytes"),
                              "vgprs_over_built_on": span_of(v["vgprs"] - v["built_on_vgprs"] for v in per.values()),
                              "sgprs_over_built_on": span_of(v["sgprs"] - v["built_on_sgprs"] for v in per.values()),
                              "valu_per_component": span_of(v["valu_per_component"] for v in per.values() if v["valu_per_component"]),
                              "built_on_valu_per_component": span_of(v["built_on_valu_per_component"] for v in per.values() if v["built_on_valu_per_component"])},
           "per_instantiation": per}
    sample = [d for k, d in desc.items() if "depth_sample_kernel" in k]
    out["sample_kernel"] = {"vgprs": int(sample[0]["next_free_vgpr"]), "sgprs": int(sample[0]["next_free_sgpr"]),
                            "lds_bytes": int(sample[0]["group_segment_fixed_size"]), "scratch_bytes": int(sample[0]["private_segment_fixed_size"])}
    out["conditions_met"] = bool(ok and out["sample_kernel"]["scratch_bytes"] == 0)
    return out


def span_of(values):
    values = list(values)
    return [min(values), max(values)]


def measure(window_s: float, rounds: int) -> dict:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import MooringSpread
    from silver2_isaacsim_amd.sea import SeaEnsemble, jonswap
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    sims = {}
    for n in SIZES:
        sc = scenes.scene_c2(n=n, margin=None)
        kw = dict(spread="cos2", seed=0, current=(0.4, 0.0, 0.0), g=sc.g)
        seas = {"ens": SeaEnsemble([jonswap(1.5, 7.0, 25.0, **kw)], n), "fd": SeaEnsemble([jonswap(1.5, 7.0, 25.0, depth=DEPTH, **kw)], n)}
        mass, pos = sc.params[:, 10].astype(np.float64), sc.state[:, 0:3].astype(np.float64)
        k, c = MooringSpread.for_body(mass, sc.dt, 3)
        phi = 2.0 * np.pi * np.arange(3) / 3.0
        anchors = np.stack([pos[:, None, 0] + 6.0 * np.cos(phi)[None, :], pos[:, None, 1] + 6.0 * np.sin(phi)[None, :],
                            np.broadcast_to(pos[:, None, 2] - 8.0, (n, 3))], axis=2)                # reach 10 m; 9.9 m of line: taut
        sim = ClosedLoopSim(sc)
        sims[n] = dict(sim=sim, seas=seas, start=(sim.cur.clone(), sim.old.clone()), variant=None,
                       spread=dict(anchors=anchors, length=9.9, stiffness=np.repeat(k[:, None], 3, axis=1), damping=np.repeat(c[:, None], 3, axis=1)))
    cases = [(n, cfg, v) for n in SIZES for cfg in CONFIGS for v in VARIANTS]

    def select(n, cfg, v):
        s = sims[n]
        if s["variant"] == (cfg, v):
            return
        s["variant"] = (cfg, v)
        sim = s["sim"]
        sim.set_sea(s["seas"][v])
        if cfg == "design":
            if sim.mooring_spread is None:
                sim.set_mooring_spread(**s["spread"])
            sim.track_extremes()
            sim.track_statistics(("z", "tension"))
        else:
            sim.clear_statistics()
            sim.clear_extremes()
            sim.clear_mooring_spread()

    def window(case, steps):
        n, cfg, v = case
        select(n, cfg, v)
        s = sims[n]
        sim = s["sim"]
        with torch.cuda.stream(sim.stream):
            sim.cur.copy_(s["start"][0]); sim.old.copy_(s["start"][1])
        sim.steps_done = 0
        if sim.extremes is not None:
            sim.extremes.reset()
        if sim.statistics is not None:
            sim.statistics.reset()
        sim.synchronize()
        t0 = time.perf_counter()
        sim.run_resident(steps, chunk=CHUNK)
        sim.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6                                  # us per physics step

    steps = {}
    for case in cases:
        window(case, 2 * CHUNK)                                                           # (first launches: code objects, clocks)
        steps[case] = 2 * CHUNK * (int(window_s / (window(case, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
        window(case, steps[case])                                                         # warm-up, discarded
    times = {case: [] for case in cases}
    for _ in range(rounds):
        for case in cases:
            times[case].append(window(case, steps[case]))
    med = {case: statistics.median(t) for case, t in times.items()}
    name = lambda case: f"{case[0]}_{case[1]}_{case[2]}"  # noqa: E731
    out = {"drag": "explicit", "chunk": CHUNK, "components": 64, "depth_m": DEPTH, "rounds": rounds,
           "steps_per_window": {name(c_): s for c_, s in steps.items()},
           "us_per_step": {name(c_): {"median": round(med[c_], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for c_, t in times.items()},
           "fd_over_ens": {str(n): {cfg: round(med[(n, cfg, "fd")] / med[(n, cfg, "ens")], 4) for cfg in CONFIGS} for n in SIZES},
           "final_state_finite": bool(all(torch.isfinite(s["sim"].cur).all() for s in sims.values()))}
    print(json.dumps(out), flush=True)
    for s in sims.values():
        s["sim"].close()
    return out


def against_expectation(m: dict) -> dict:
    """The measured ratios beside what EXPECTATION said of them: 1.11 .. 1.14 bare and 1.09 .. 1.13 in the design configuration at
    1 048 576 bodies, no more than the upper ends at 4 096."""
    out = {}
    for n, ratios in m["fd_over_ens"].items():
        for cfg, r in ratios.items():
            hi = 1.14 if cfg == "bare" else 1.13
            lo = (1.11 if cfg == "bare" else 1.09) if int(n) == SIZES[1] else 1.0
            out[f"{n}_{cfg}"] = {"measured": r, "expected": [lo, hi], "within": bool(lo <= r <= hi), "measured_over_expected_upper": round(r / hi, 4)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa-only", action="store_true", help="read the generated code only (no GPU)")
    ap.add_argument("--asm", default=None, help="a hipcc -S listing of csrc/hydro_kernels.hip to read instead of compiling one")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    data["expectation"] = EXPECTATION
    if args.isa_only:
        data["isa"] = isa(args.asm)
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_sea_depth.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["sample_kernel"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"one sim per size, explicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the same initial state and step count 0 with the records reset, ending in a stream synchronise; "
                            f"variants alternate within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds)
        data["against_expectation"] = against_expectation(data["measurements"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
