#!/usr/bin/env python3
"""What a sheared current costs in the resident closed loop: hydro_step_fused_tiled_multi_shear - sheared_water, the knot loop
behind depth_water in every step - against the kernels this feature leaves byte-identical (the _fd kernels under the same
finite-depth sea), measured on the same bodies in the same run.

  python scripts/diag_current_profile.py              (GPU)  C2 buoys, 16 knots -> profiles/current_profile.json
  python scripts/diag_current_profile.py --isa-only   (no GPU) registers, LDS and scratch of the 64 instantiations beside the _fd kernels
                                                             they are built on, and the instructions of every knot loop, from hipcc -S
                                                             (--asm FILE: a listing at hand)

Two configurations, explicit drag, nothing but the water: "current_only" (one member without components over a depth of 20 m: the
step is the bare one plus the water's bookkeeping) and "full_sea" (a JONSWAP sea of 64 components at that depth).
Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, at 4 096 and 1 048 576 bodies:
  fd     no profile: the parent's _fd kernels - the baseline
  shear  set_current_profile(a 16-knot power law plus nothing else): the new kernels
Protocol (that of scripts/diag_sea_depth.py): every timed window starts from the same initial state and step count 0, lasts at
least --window seconds of back-to-back launches of run_resident(chunk=64) and ends in a stream synchronise; the variants alternate
within each of --rounds rounds, after a warm-up window each, and the order of the cases ROTATES from round to round (a case that
always runs behind the heaviest window reads slow).  Reported: the median over the rounds and the range, in us per physics step.
No ratio is gated.  The expectation written down beforehand is EXPECTATION."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "current_profile.json")
CHUNK = 64
SIZES = (4096, 1048576)
DEPTH = 20.0
KNOTS = 16
CONFIGS = ("current_only", "full_sea")
VARIANTS = ("fd", "shear")
FAMILIES = {"step_fused_multi_shear_tiled_kernel": "step_fused_multi_fd_tiled_kernel",
            "step_fused_multi_shear_stat_tiled_kernel": "step_fused_multi_fd_stat_tiled_kernel"}
EXPECTATION = ("from the code, before any measurement: sheared_water adds behind depth_water one clamp pair to re-form zc (the compiler should "
               "share it with depth_water's), then per segment a subtraction, a product, two clamps and three fmas - about 6 VALU per segment, "
               "about 95 at 16 knots - and three adds; the knot records arrive through scalar loads of 32 B per segment.  A bare step is about "
               "530 VALU instructions and a step through 64 finite-depth components about 3 200, so where the step is bound by VALU issue the "
               "profile should cost (530 + 95) / 530 = 1.18 times the current-only step and (3 200 + 95) / 3 200 = 1.03 times the step in a full "
               "sea, at 1 048 576 bodies; less at 4 096 bodies, where 64 tiles leave three quarters of the CUs idle and a step is latency - there "
               "the 15 dependent trips of the knot loop, each behind a scalar load, may show instead.  Registers: the loop's values are dead once "
               "u is formed, so the kernels should stay within a few VGPRs of the _fd kernels' 158-165, at 3 waves per SIMD, without scratch; "
               "SGPRs at the 100 they stand at; LDS the _fd kernels'")


def isa(asm_path=None) -> dict:
    """Over the 2 x 32 instantiations: VGPRs, SGPRs, LDS bytes and scratch beside the _fd instantiation of the same flags; and of EVERY
    instantiation the knot loop - the loop inside the step loop whose product carries the clamp - with its instructions by kind."""
    from scripts import isa_mix
    asm = open(asm_path).read() if asm_path else isa_mix.assembly()
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M)}

    def knot_loops(name):
        body, loops = bodies[name], []
        for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(?:\s*;[^\n]*\n)*", body, re.M):      # a label with the comment lines that follow it
            if "Loop Header" not in m.group(0):
                continue
            back = [b.end() for b in re.finditer(r"^\s+s_c?branch\S* " + re.escape(m.group(1)) + r"$", body, re.M)]
            text = body[m.start():max(back)] if back else ""
            lines = [l.split(";")[0].strip() for l in text.splitlines()[1:]]
            lines = [l for l in lines if l and not l.endswith(":")]
            if any(l.startswith(("v_cos_f32", "s_cbranch_execz", "s_cbranch_execnz")) for l in lines) or not any(re.match(r"v_mul_f32\S* .* clamp$", l) for l in lines):
                continue
            op = [l.split()[0] for l in lines]
            loops.append({"instructions": len(op), "valu": sum(o.startswith("v_") for o in op), "scalar_loads": sum(o.startswith("s_load") for o in op),
                          "scalar_alu_and_branch": sum(o.startswith("s_") and not o.startswith("s_load") for o in op),
                          "lds": sum(o.startswith("ds_") for o in op),
                          "vector_memory": sum(o.startswith(("global_", "flat_", "buffer_", "scratch_")) for o in op)})
        return loops

    per, ok = {}, True
    for new, base in FAMILIES.items():
        mine = {flags_of(k): (k, d) for k, d in desc.items() if re.search(r"\d" + new + "I", k)}
        theirs = {flags_of(k): (k, d) for k, d in desc.items() if re.search(r"\d" + base + "I", k)}
        ok = ok and len(mine) == 32
        for flags, (name, d) in sorted(mine.items()):
            vgprs, loops = int(d["next_free_vgpr"]), knot_loops(name)
            _, base_d = theirs[flags]
            row = {"vgprs": vgprs, "built_on_vgprs": int(base_d["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
                   "built_on_sgprs": int(base_d["next_free_sgpr"]), "waves_per_simd": 512 // (-(-vgprs // 8) * 8),
                   "lds_bytes": int(d["group_segment_fixed_size"]), "built_on_lds_bytes": int(base_d["group_segment_fixed_size"]),
                   "scratch_bytes": int(d["private_segment_fixed_size"]), "knot_loops": loops}
            ok = ok and (row["scratch_bytes"] == 0 and vgprs <= 168 and row["waves_per_simd"] >= 3 and row["lds_bytes"] == row["built_on_lds_bytes"]
                         and len(loops) == 1 and loops[0]["scalar_loads"] > 0 and loops[0]["lds"] == 0 and loops[0]["vector_memory"] == 0)
            per[new + "<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags)) + ">"] = row
    span = lambda key: span_of(v[key] for v in per.values())  # noqa: E731
    out = {"instantiations": {"count": len(per), "vgprs": span("vgprs"), "built_on_vgprs": span("built_on_vgprs"), "sgprs": span("sgprs"),
                              "built_on_sgprs": span("built_on_sgprs"), "lds_bytes": span("lds_bytes"), "scratch_bytes": span("scratch_bytes"),
                              "vgprs_over_built_on": span_of(v["vgprs"] - v["built_on_vgprs"] for v in per.values()),
                              "knot_loop_valu_per_segment": span_of(l["valu"] for v in per.values() for l in v["knot_loops"]),
                              "knot_loop_scalar_loads": span_of(l["scalar_loads"] for v in per.values() for l in v["knot_loops"])},
           "per_instantiation": per}
    name = [k for k in desc if "shear_sample_kernel" in k][0]
    sample = desc[name]
    out["sample_kernel"] = {"vgprs": int(sample["next_free_vgpr"]), "sgprs": int(sample["next_free_sgpr"]), "lds_bytes": int(sample["group_segment_fixed_size"]),
                            "scratch_bytes": int(sample["private_segment_fixed_size"]), "knot_loops": knot_loops(name)}
    out["conditions_met"] = bool(ok and out["sample_kernel"]["scratch_bytes"] == 0 and len(out["sample_kernel"]["knot_loops"]) == 1)
    return out


def span_of(values):
    values = list(values)
    return [min(values), max(values)] if values else None


def measure(window_s: float, rounds: int) -> dict:
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.sea import CurrentProfile, SeaEnsemble, SeaSpectrum, jonswap
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    profile = CurrentProfile.power_law(0.4, 0.0, DEPTH, knots=KNOTS)
    sims = {}
    for n in SIZES:
        sc = scenes.scene_c2(n=n, margin=None)
        seas = {"current_only": SeaEnsemble([SeaSpectrum((0.4, 0.0, 0.0), DEPTH)], n),
                "full_sea": SeaEnsemble([jonswap(1.5, 7.0, 25.0, depth=DEPTH, spread="cos2", seed=0, current=(0.4, 0.0, 0.0), g=sc.g)], n)}
        sim = ClosedLoopSim(sc)
        sims[n] = dict(sim=sim, seas=seas, start=(sim.cur.clone(), sim.old.clone()), variant=None)
    cases = [(n, cfg, v) for n in SIZES for cfg in CONFIGS for v in VARIANTS]

    def select(n, cfg, v):
        s = sims[n]
        if s["variant"] == (cfg, v):
            return
        sim = s["sim"]
        if s["variant"] is None or s["variant"][0] != cfg:
            sim.set_sea(s["seas"][cfg])
        if v == "shear":
            sim.set_current_profile(profile)
        else:
            sim.clear_current_profile()
        s["variant"] = (cfg, v)

    def window(case, steps):
        n, cfg, v = case
        select(n, cfg, v)
        s = sims[n]
        sim = s["sim"]
        with torch.cuda.stream(sim.stream):
            sim.cur.copy_(s["start"][0]); sim.old.copy_(s["start"][1])
        sim.steps_done = 0
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
    for r in range(rounds):
        for case in cases[r % len(cases):] + cases[:r % len(cases)]:                      # the order rotates from round to round
            times[case].append(window(case, steps[case]))
    med = {case: statistics.median(t) for case, t in times.items()}
    name = lambda case: f"{case[0]}_{case[1]}_{case[2]}"  # noqa: E731
    out = {"drag": "explicit", "chunk": CHUNK, "components": {"current_only": 0, "full_sea": 64}, "knots": KNOTS, "depth_m": DEPTH, "rounds": rounds,
           "steps_per_window": {name(c_): s for c_, s in steps.items()},
           "us_per_step": {name(c_): {"median": round(med[c_], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for c_, t in times.items()},
           "shear_over_fd": {str(n): {cfg: round(med[(n, cfg, "shear")] / med[(n, cfg, "fd")], 4) for cfg in CONFIGS} for n in SIZES},
           "final_state_finite": bool(all(torch.isfinite(s["sim"].cur).all() for s in sims.values()))}
    print(json.dumps(out), flush=True)
    for s in sims.values():
        s["sim"].close()
    return out


def against_expectation(m: dict) -> dict:
    """The measured ratios beside what EXPECTATION said of them: about 1.18 current-only and about 1.03 in a full sea at 1 048 576
    bodies, no more than that at 4 096."""
    out = {}
    for n, ratios in m["shear_over_fd"].items():
        for cfg, r in ratios.items():
            expected = 1.18 if cfg == "current_only" else 1.03
            out[f"{n}_{cfg}"] = {"measured": r, "expected": expected if int(n) == SIZES[1] else [1.0, expected],
                                 "measured_over_expected": round(r / expected, 4)}
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
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_current_profile.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["sample_kernel"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"one sim per size, explicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the same initial state and step count 0, ending in a stream synchronise; variants alternate within "
                            f"each of {args.rounds} rounds after one warm-up window each, the order of the cases rotating from round to round")
        data["measurements"] = measure(args.window, args.rounds)
        data["against_expectation"] = against_expectation(data["measurements"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
