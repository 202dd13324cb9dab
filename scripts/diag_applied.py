#!/usr/bin/env python3
"""What the applied wrench costs in the resident closed loop (hydro_step_fused_tiled_multi_app against the unchanged
hydro_step_fused_tiled_multi), measured on the GPU and counted in the assembly.

  python scripts/diag_applied.py              (GPU)  run_resident(chunk=64) at 19 456 and 1 048 576 bodies: plain, world frame,
                                                     body frame, each with explicit and implicit drag -> profiles/applied_wrench.json
  python scripts/diag_applied.py --isa-only   (no GPU) only the VALU instructions per step of the three loops, from hipcc -S

Protocol: the three variants of a (size, drag) pair are sims of the same scene (C2 buoys, no branch-margin gating; the
push is horizontal, 1 N per kg, with a yaw torque, so that the submersion of the bodies - which decides the branches the
wrench takes - stays what it is without the push).  Every timed window starts from the same initial state, lasts at least
--window seconds of back-to-back 64-step launches and ends in a stream synchronise; the variants alternate within each of
--rounds rounds, after a warm-up window each.  Reported: the median over the rounds and the spread (min, max)."""
import argparse
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "applied_wrench.json")
CHUNK = 64
SIZES = (19456, 1048576)
VARIANTS = ("plain", "world", "body")


def valu_per_step() -> dict:
    """VALU instructions of one trip through the step loop of the <f32, temporal, no KE, Numba> instantiations.  The applied
    kernel's loop holds both frames behind one scalar branch: the body-frame block is what follows that branch up to the
    next label, the world-frame block the label after it."""
    from scripts import isa_mix
    asm = isa_mix.assembly()
    valu = lambda text: sum(isa_mix.classify(op) != "not-valu" for op in re.findall(r"^\s+([a-z][a-z0-9_]+)", text, re.M))  # noqa: E731
    out = {}
    for drag, flag in (("explicit", 0), ("implicit", 1)):
        loops = {}
        for name in ("step_fused_multi_tiled_kernel", "step_fused_multi_rec_tiled_kernel", "step_fused_multi_app_tiled_kernel"):
            body = re.search(r"^(_Z\S*" + name + f"ILb0ELb0ELb{flag}ELb0ELb0E" + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
            loops[name] = re.search(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)^\s+s_branch \1$", body, re.S | re.M).group(2)
        app = loops["step_fused_multi_app_tiled_kernel"]
        blocks = re.split(r"^\.LBB\d+_\d+:[^\n]*\n", app, flags=re.M)
        fork = next(i for i, b in enumerate(blocks) if "s_cbranch_vccz" in b and "s_cbranch_execnz" in b)
        body_only, world_only = valu(blocks[fork].split("s_cbranch_vccz")[1]), valu(blocks[fork + 1])
        out[drag] = {"plain": valu(loops["step_fused_multi_tiled_kernel"]), "plain with recorder": valu(loops["step_fused_multi_rec_tiled_kernel"]),
                     "world": valu(app) - body_only, "body": valu(app) - world_only}
    return out


def measure(window_s: float, rounds: int, sizes) -> list:
    import numpy as np
    import torch
    from silver2_isaacsim_amd import scenes
    from silver2_isaacsim_amd.simulate import ClosedLoopSim
    assert torch.cuda.is_available(), "the measurement needs the GPU (no fallback)"
    results = []
    for n in sizes:
        sc = scenes.scene_c2(n=n, margin=None)
        rng = np.random.default_rng(5)
        m = sc.params[:, 10:11].astype(np.float64)
        push = np.zeros((n, 6), np.float32)
        push[:, 0:2] = rng.uniform(-1, 1, (n, 2)) * m
        push[:, 5] = rng.uniform(-1, 1, n) * 0.1 * m[:, 0]
        for implicit in (False, True):
            sims = {v: ClosedLoopSim(sc, implicit_drag=implicit) for v in VARIANTS}
            for v in ("world", "body"):
                sims[v].set_applied_wrench(push, frame=v)
            start = {v: (s.cur.clone(), s.old.clone()) for v, s in sims.items()}

            def window(v, launches):
                s = sims[v]
                with torch.cuda.stream(s.stream):
                    s.cur.copy_(start[v][0]); s.old.copy_(start[v][1])
                s.synchronize()
                t0 = time.perf_counter()
                s.run_resident(launches * CHUNK, chunk=CHUNK)
                s.synchronize()
                return (time.perf_counter() - t0) / (launches * CHUNK) * 1e6                # us per physics step

            window("plain", 4)                                                                # (first launches: code objects, clocks)
            launches = 2 * (int(window_s / (window("plain", 8) * CHUNK * 1e-6)) // 2 + 1)      # even: the ping-pong ends where it began
            for v in VARIANTS:
                window(v, launches)                                                           # warm-up, discarded
            times = {v: [] for v in VARIANTS}
            for _ in range(rounds):
                for v in VARIANTS:
                    times[v].append(window(v, launches))
            finite = {v: bool(torch.isfinite(s.cur).all()) for v, s in sims.items()}
            med = {v: statistics.median(t) for v, t in times.items()}
            row = {"bodies": n, "drag": "implicit" if implicit else "explicit", "chunk": CHUNK, "launches_per_window": launches, "rounds": rounds,
                   "us_per_step": {v: {"median": round(med[v], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for v, t in times.items()},
                   "over_plain_percent": {v: round(100.0 * (med[v] / med["plain"] - 1.0), 2) for v in ("world", "body")},
                   "final_state_finite": finite}
            print(json.dumps(row), flush=True)
            results.append(row)
            for s in sims.values():
                s.close()
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
        data["valu_per_step"] = valu_per_step()
        print(json.dumps(data["valu_per_step"]))
    else:
        import torch
        data["device"] = torch.cuda.get_device_name(0)
        data["protocol"] = (f"run_resident(chunk={CHUNK}); windows of >= {args.window} s from the same initial state, ending in a stream "
                            f"synchronise; variants alternate within each of {args.rounds} rounds after one warm-up window each")
        data["measurements"] = measure(args.window, args.rounds, args.sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)
    return data


if __name__ == "__main__":
    main()
