#!/usr/bin/env python3
"""What tethers cost in the resident closed loop: hydro_step_fused_tiled_multi_teth with a record in which nobody is tethered
(every wave skips the evaluation on a ballot) and with everybody tethered and taut (every wave exchanges six values between
its lanes and evaluates the line), against the loops that exist without tethers - the plain resident loop
(hydro_step_fused_tiled_multi) and the loop with mooring lines, 8 wave components, a pose hold and a bed (_multi_moor), whose
kernels this feature leaves byte-identical: the baseline, measured in the same run.

  python scripts/diag_tether.py              (GPU)  C2 buoys at 4 096, 19 456 and 1 048 576 bodies -> profiles/tether.json
  python scripts/diag_tether.py --isa-only   (no GPU) VALU, LDS, ds_bpermute and global-load instructions per step of the loops,
                                                    registers, LDS and scratch of the 32 instantiations, from hipcc -S

Variants, ONE sim per size (the same buffers, the same engine), switched between the timed windows:
  plain                  run_resident(chunk=64), still water
  teth_none              set_tether with no pairs: the new kernel, every option absent, every wave skipping
  teth_taut              bodies 2 i and 2 i + 1 tied by a line half as long as their distance, the default constants of the pair (in still
                         water the pairs draw together within a window and the lines end slack: the share that still pulls is reported,
                         and the waves evaluate the line either way)
  moor_w8_ctl_bed        every body on a taut mooring line, 8 wave components, a depth hold and a bed at z = -1000 m
  moor_w8_ctl_bed_none   the same through the new kernel with nobody tethered
  moor_w8_ctl_bed_taut   the same with everybody tethered and taut
Protocol (that of scripts/diag_extremes.py): every timed window starts from the same initial state and step count 0, lasts at
least --window seconds of back-to-back launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max), in us per
physics step, and each tethered variant over its baseline.  No ratio is fixed in advance; the one expectation: the untethered
scene should cost visibly less than the taut one, or the skip is not working."""

import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "tether.json")
CHUNK = 64
SIZES = (4096, 19456, 1048576)
VARIANTS = ("plain", "teth_none", "teth_taut", "moor_w8_ctl_bed", "moor_w8_ctl_bed_none", "moor_w8_ctl_bed_taut")
PAIRS = (("teth_none", "plain"), ("teth_taut", "plain"), ("teth_taut", "teth_none"), ("moor_w8_ctl_bed_none", "moor_w8_ctl_bed"),
         ("moor_w8_ctl_bed_taut", "moor_w8_ctl_bed"), ("moor_w8_ctl_bed_taut", "moor_w8_ctl_bed_none"))
KP, KD = 25.0, 10.0
Z_FAR = -1000.0
KERNELS = ("step_fused_multi_tiled_kernel", "step_fused_multi_ext_tiled_kernel", "step_fused_multi_teth_tiled_kernel")


def isa() -> dict:
    """Of the <f32, temporal, no KE, Numba> instantiations, per drag form: the instructions of the step loop, every branch of it
    counted (each optional policy stands behind a scalar branch of its own, the tether's evaluation behind its ballot).  And
    over the 32 instantiations of the tether kernel: VGPRs, SGPRs, LDS bytes, scratch - each of them listed, beside the LDS of
    the extremes kernel's instantiation of the same flags."""
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
                         "lds_reads": sum(op.startswith("ds_read") for op in loop), "lds_writes": sum(op.startswith("ds_write") for op in loop),
                         "ds_bpermute": sum(op.startswith("ds_bpermute") for op in loop),
                         "global_loads": sum(op.startswith("global_load") for op in loop)}
        row["tether_over_extremes"] = {k: row[KERNELS[2]][k] - row[KERNELS[1]][k] for k in ("valu", "transcendental", "lds_reads", "lds_writes", "ds_bpermute", "global_loads")}
        out["loop"][drag] = row
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if KERNELS[1] in m.group(1) or KERNELS[2] in m.group(1)}
    teth = {k: d for k, d in desc.items() if KERNELS[2] in k}
    span = lambda key: [min(int(d[key]) for d in teth.values()), max(int(d[key]) for d in teth.values())]  # noqa: E731
    out["instantiations"] = {"count": len(teth), "vgprs": span("next_free_vgpr"), "sgprs": span("next_free_sgpr"),
                             "lds_bytes": span("group_segment_fixed_size"), "scratch_bytes": span("private_segment_fixed_size")}
    flags_of = lambda name: re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()  # noqa: E731
    ext_of = {flags_of(k): d for k, d in desc.items() if KERNELS[1] in k}
    per = {}
    for name, d in teth.items():
        flags = flags_of(name)
        ext = ext_of[flags]
        vgprs = int(d["next_free_vgpr"])
        per["<" + ", ".join(f"{k}={v}" for k, v in zip(("HALF", "NT", "IMPLICIT", "KE", "WARP"), flags)) + ">"] = {
            "vgprs": vgprs, "waves_per_simd": 512 // (-(-vgprs // 8) * 8), "lds_bytes": int(d["group_segment_fixed_size"]),
            "ext_kernel_lds_bytes": int(ext["group_segment_fixed_size"]), "scratch_bytes": int(d["private_segment_fixed_size"])}
    out["per_instantiation"] = dict(sorted(per.items()))
    out["conditions_met"] = all(v["scratch_bytes"] == 0 and v["vgprs"] <= 168 and v["waves_per_simd"] >= 3 and v["lds_bytes"] <= v["ext_kernel_lds_bytes"]
                                for v in per.values()) and len(per) == 32
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from scripts.diag_sea import sea_of
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.mooring import Mooring
    from silver2_isaacsim_amd.seabed import Seabed
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    from silver2_isaacsim_amd.tether import Tether
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        mass = sc.params[:, 10:11].astype(np.float64)
        zero = np.zeros_like(mass)
        far = Seabed.for_step(Z_FAR, sc.dt)
        k, c = Mooring.for_body(mass[:, 0], sc.dt)
        anchors = sc.state[:, 0:3].astype(np.float64) - np.array([0.0, 0.0, 5.0])
        a = np.arange(0, n - 1, 2)
        pairs = np.stack([a, a + 1], axis=1)
        tk, tc = Tether.for_pair(mass[a, 0], mass[a + 1, 0], sc.dt)
        apart = np.linalg.norm(sc.state[a + 1, 0:3].astype(np.float64) - sc.state[a, 0:3], axis=1)
        nobody = np.zeros((0, 2), np.int64)
        sim = ClosedLoopSim(sc, implicit_drag=True)
        start = (sim.cur.clone(), sim.old.clone())
        state = {"variant": None}

        def select(v):
            if state["variant"] == v:
                return
            state["variant"] = v
            sim.synchronize()
            full = v.startswith("moor_w8_ctl_bed")
            if full:
                sim.set_sea(sea_of(8))
                sim.set_pose_hold(position=sc.state[:, 0:3], kp_lin=np.concatenate([zero, zero, mass * KP], axis=1),
                                  kd_lin=np.concatenate([zero, zero, mass * KD], axis=1))
                sim.set_seabed(far)
                sim.set_mooring(anchors, length=4.9, stiffness=k, damping=c)
            else:
                sim.clear_sea()
                sim.clear_pose_hold()
                sim.clear_seabed()
                sim.clear_mooring()
            if v.endswith("_none"):
                sim.set_tether(nobody, length=1.0, stiffness=0.0)
            elif v.endswith("_taut"):
                sim.set_tether(pairs, length=0.5 * apart, stiffness=tk, damping=tc)
            else:
                sim.clear_tether()

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

        steps, pulling = {}, {}
        for v in VARIANTS:
            window(v, 2 * CHUNK)                                                          # (first launches: code objects, clocks)
            steps[v] = 2 * CHUNK * (int(window_s / (window(v, 2 * CHUNK) * 2 * CHUNK * 1e-6)) + 1)   # even launches: the ping-pong ends where it began
            window(v, steps[v])                                                           # warm-up, discarded
            if sim.tether is not None:
                probe = scenes.from_tiled(sim.engine.tether_wrench(sim.cur, sim.tether, n).cpu().numpy(), n)
                pulling[v] = float(probe.any(axis=1).mean())                              # share of the bodies whose tether pulls at the end of a window
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                times[v].append(window(v, steps[v]))
        med = {v: statistics.median(t) for v, t in times.items()}
        row = {"bodies": n, "drag": "implicit", "chunk": CHUNK, "steps_per_window": steps, "rounds": rounds,
               "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
               "ratios": {f"{a_}_over_{b_}": round(med[a_] / med[b_], 4) for a_, b_ in PAIRS},
               "share_pulling_at_the_end_of_a_window": pulling,
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
        data.setdefault("measurements", "not measured: no timing has been taken on an MI355X yet (python scripts/diag_tether.py)")
        print(json.dumps(data["isa"]["instantiations"]), json.dumps(data["isa"]["loop"]), data["isa"]["conditions_met"])
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
