#!/usr/bin/env python3
"""What an irregular sea costs in the resident closed loop: hydro_step_fused_tiled_multi_irr with 8, 16, 32 and 64 wave
components - every lane evaluates every component, in a loop unrolled in groups of four that reads the table with scalar loads -
against the regular sea of 8 components, whose kernels this feature leaves byte-identical: the baseline, measured in the same run.

  python scripts/diag_sea_spectrum.py              (GPU)  C2 buoys at 4 096 and 1 048 576 bodies -> profiles/sea_spectrum.json
  python scripts/diag_sea_spectrum.py --isa-only   (no GPU) registers, LDS and scratch of the 32 instantiations, and the instructions
                                                          of the component loops of one of them, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows, explicit drag:
  sea8              set_sea(SeaState of 8 components): the parent's path, the sea kernel with its 8 components unrolled
  irr8 .. irr64     set_sea(SeaSpectrum of the first 8, 16, 32, 64 of the same components): the _irr kernel
  sea8_spread_ext   the regular sea, a three-line spread and the extremes: the parent's spread kernel
  irr64_spread_ext  64 components with the same spread and extremes
Protocol (that of scripts/diag_sea.py): every timed window starts from the same initial state and step
count 0, lasts at least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate
within each of --rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max),
in us per physics step.  No ratio is gated.  The expectation written down beforehand is EXPECTATION."""
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
OUT = os.path.join(REPO, "profiles", "sea_spectrum.json")
CHUNK = 64
SIZES = (4096, 1048576)
VARIANTS = ("sea8", "irr8", "irr16", "irr32", "irr64", "sea8_spread_ext", "irr64_spread_ext")
PAIRS = (("irr8", "sea8"), ("irr16", "sea8"), ("irr32", "sea8"), ("irr64", "sea8"), ("irr64", "irr8"), ("irr64_spread_ext", "sea8_spread_ext"))
KERNELS = ("step_fused_multi_spread_tiled_kernel", "step_fused_multi_irr_tiled_kernel")
EXPECTATION = ("a component costs 37 VALU instructions in the two passes together (15 + 22, 10 of them fp64 and 4 transcendental), where the "
               "unrolled regular sea paid about 40 for its one pass and a half; the step without a sea is about 530 VALU instructions, so where the "
               "loop is bound by VALU issue 8 components should cost about what the regular sea costs (within 10 %: the _irr kernel is of the "
               "spread family, with its optional policies' branches), and 64 components about (530 + 64 * 37) / (530 + 8 * 40) = 3.4 times the "
               "8-component sea, less where launch overhead or memory hides arithmetic (4 096 bodies), more if the scalar loads of a group are "
               "not hidden by the two other waves of the SIMD")


def sea_of(waves: int, spectrum: bool):
    """A 0.3 m/s current and the first `waves` of 64 components of equal amplitude (hs = 1 m at 64), wavelengths 200 m down to 6 m,
    headings fanned by the golden angle."""
    from silver2_isaacsim_amd.sea import SeaSpectrum, SeaState
    sea = (SeaSpectrum if spectrum else SeaState)((0.3, -0.1, 0.0))
    for j in range(waves):
        kappa = 2.0 * math.pi / (200.0 * (6.0 / 200.0) ** (((j * 37) % 64) / 63.0))
        head = math.radians(137.50776405003785 * j)
        sea.add_wave(1.0 / math.sqrt(8.0 * 64), kappa * math.cos(head), kappa * math.sin(head), math.sqrt(9.81 * kappa), 0.7 * j)
    return sea


def isa() -> dict:
    """Over the 32 instantiations of the _irr kernel: VGPRs, SGPRs, LDS bytes and scratch, each beside the spread kernel's
    instantiation of the same flags.  And of the <f32, temporal, explicit, no KE, Numba> instantiation: the COMPONENT LOOPS - the
    depth-2 loops inside the step loop that hold a v_cos_f32 - each with the components a trip evaluates and its instruction mix."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    ops = lambda text: re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M)  # noqa: E731
    kind = lambda op, what: isa_mix.classify(op) == what  # noqa: E731
    body = re.search(r"^(_Z\S*" + KERNELS[1] + r"ILb0ELb0ELb0ELb0ELb0E[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
    loops = []
    for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(?:\s*;[^\n]*\n)*", body, re.M):       # a label with the comment lines that follow it
        if "Loop Header: Depth=2" not in m.group(0):
            continue
        back = [b.end() for b in re.finditer(r"^\s+s_c?branch\S* " + re.escape(m.group(1)) + r"$", body, re.M)]
        text = body[m.start():max(back)] if back else ""
        loop = ops(text)
        if "v_cos_f32_e32" not in loop:
            continue
        cos = sum(op.startswith("v_cos_f32") for op in loop)
        loops.append({"pass": "velocity" if any(op.startswith("v_exp_f32") for op in loop) else "elevation", "components_per_trip": cos,
                      "instructions": len(loop), "valu": sum(not kind(op, "not-valu") for op in loop), "fp64": sum(kind(op, "fp64 arithmetic") for op in loop),
                      "transcendental": sum(kind(op, "transcendental") for op in loop),
                      "scalar_loads": sum(op.startswith("s_load") for op in loop), "scalar_waits": sum(op == "s_waitcnt" for op in loop),
                      "lds": sum(op.startswith("ds_") for op in loop), "global_memory": sum(op.startswith("global_") for op in loop),
                      "scratch": sum(op.startswith("scratch_") for op in loop)})
    out = {"table_read": "scalar loads (s_load_dwordx8 / x4 / x2 through address_space(4)), the loop unrolled in groups of four: no LDS staging",
           "component_loops": loops}
    single = {p: [l for l in loops if l["pass"] == p and l["components_per_trip"] == 1] for p in ("elevation", "velocity")}
    if all(len(v) == 1 for v in single.values()):
        out["valu_per_component"] = {p: v[0]["valu"] for p, v in single.items()}
        out["valu_per_component"]["both_passes"] = sum(out["valu_per_component"].values())
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if any(k in m.group(1) for k in KERNELS)}
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    spread_of = {flags_of(k): d for k, d in desc.items() if KERNELS[0] in k}
    irr = {k: d for k, d in desc.items() if KERNELS[1] in k}
    span = lambda key: [min(int(d[key]) for d in irr.values()), max(int(d[key]) for d in irr.values())]  # noqa: E731
    out["instantiations"] = {"count": len(irr), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    per = {}
    for name, d in irr.items():
        spread = spread_of[flags_of(name)]
        vgprs = int(d["next_free_vgpr"])
        per["<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags_of(name))) + ">"] = {
            "vgprs": vgprs, "spread_kernel_vgprs": int(spread["next_free_vgpr"]), "sgprs": int(d["next_free_sgpr"]),
            "waves_per_simd": 512 // (-(-vgprs // 8) * 8), "lds_bytes": int(d["group_segment_fixed_size"]),
            "spread_kernel_lds_bytes": int(spread["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
    out["per_instantiation"] = dict(sorted(per.items()))
    out["conditions_met"] = (len(per) == 32 and all(v["scratch_bytes"] == 0 and v["vgprs"] <= 168 and v["waves_per_simd"] >= 3
                                                    and v["lds_bytes"] == v["spread_kernel_lds_bytes"] for v in per.values())
                             and len(loops) == 4 and all(l["lds"] == 0 and l["global_memory"] == 0 and l["scratch"] == 0 for l in loops))
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import MooringSpread
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    seas = {"sea8": sea_of(8, False), **{f"irr{k}": sea_of(k, True) for k in (8, 16, 32, 64)}}
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10].astype(np.float64)
        pos = sc.state[:, 0:3].astype(np.float64)
        k, c = MooringSpread.for_body(mass, sc.dt, 3)
        phi = 2.0 * np.pi * np.arange(3) / 3.0
        anchors = np.stack([pos[:, None, 0] + 6.0 * np.cos(phi)[None, :], pos[:, None, 1] + 6.0 * np.sin(phi)[None, :],
                            np.broadcast_to(pos[:, None, 2] - 8.0, (n, 3))], axis=2)                # reach 10 m; 9.9 m of line: taut
        three = dict(anchors=anchors, length=9.9, stiffness=np.repeat(k[:, None], 3, axis=1), damping=np.repeat(c[:, None], 3, axis=1))
        sim = ClosedLoopSim(sc)
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.set_sea(seas[v.split("_")[0]])
            if v.endswith("_spread_ext"):
                if sim.mooring_spread is None:
                    sim.set_mooring_spread(**three)
                    sim.track_extremes()
            else:
                sim.clear_mooring_spread()
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
        row = {"bodies": n, "drag": "explicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "ratios": {f"{a_}_over_{b_}": round(med[a_] / med[b_], 4) for a_, b_ in PAIRS},
               "us_per_step_per_added_component": round((med["irr64"] - med["irr8"]) / 56.0, 5),
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
    data["expectation"] = EXPECTATION
    if args.isa_only:
        data["isa"] = isa()
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_sea_spectrum.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["component_loops"]), data["isa"]["conditions_met"])
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"one sim per size, explicit drag, run_resident(chunk={CHUNK}), the variant switched between windows; windows of >= "
                            f"{args.window} s from the same initial state and step count 0, ending in a stream synchronise; variants alternate within "
                            f"each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
