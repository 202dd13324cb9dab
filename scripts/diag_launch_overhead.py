#!/usr/bin/env python3
"""DEV-ONLY: host cost of one step call (4 096 bodies) - engine method vs the raw ctypes call with prebuilt
arguments vs the prepared call, then the calls the closed loop (fused steps) and the plugin (prepared
array-of-structs step, 20 bodies) issue.   python scripts/diag_launch_overhead.py"""
import ctypes, os, sys, time
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from silver2_isaacsim_amd import scenes, _native as nat
from silver2_isaacsim_amd.engine import HydroEngine
dev = torch.device("cuda:0")
sc = scenes.scene_c2()
eng = HydroEngine(sc.n, dev, sc.rho, sc.g); eng.set_params(sc.params)
S = torch.from_numpy(scenes.to_tiled(sc.state)).to(dev); P = torch.from_numpy(scenes.to_tiled(sc.prev)).to(dev)
O = eng.alloc_tiled(6, sc.n)
stream = torch.cuda.Stream(dev)


def bench(fn, k=20000):
    with torch.cuda.stream(stream):
        for _ in range(200): fn()
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(k): fn()
        t_issue = time.perf_counter() - t0
        stream.synchronize()
        t_all = time.perf_counter() - t0
    return t_issue / k * 1e6, t_all / k * 1e6


with torch.cuda.stream(stream):
    a = bench(lambda: eng.step_wrench_tiled(S, sc.n, sc.dt, out=O, prev=P))
    print(f"engine.step_wrench_tiled      host issue {a[0]:6.2f} us/call   wall {a[1]:6.2f} us/step")
    lib = eng._lib
    args = (eng._h, ctypes.c_int64(sc.n), ctypes.c_void_p(S.data_ptr()), ctypes.c_int64(13 * 64), ctypes.c_void_p(P.data_ptr()),
            ctypes.c_int64(6 * 64), ctypes.c_double(sc.dt), ctypes.c_void_p(O.data_ptr()), ctypes.c_int64(6 * 64),
            ctypes.c_void_p(stream.cuda_stream))
    fn = lib.hydro_step_wrench_tiled
    b = bench(lambda: fn(*args))
    print(f"raw ctypes, prebuilt args     host issue {b[0]:6.2f} us/call   wall {b[1]:6.2f} us/step")
    if hasattr(eng, "prepare_step_wrench_tiled"):
        step = eng.prepare_step_wrench_tiled(S, sc.n, sc.dt, out=O, prev=P, stream=stream)
        c = bench(step)
        print(f"prepared step                 host issue {c[0]:6.2f} us/call   wall {c[1]:6.2f} us/step")
    # the closed loop's unprepared calls: two state buffers in ping-pong (the result is not looked at)
    S2 = S.clone()
    d = bench(lambda: eng.step_fused_tiled(S, S2, sc.n, sc.dt))
    print(f"engine.step_fused_tiled       host issue {d[0]:6.2f} us/call   wall {d[1]:6.2f} us/step")
    e = bench(lambda: eng.step_fused_tiled_multi(S, S2, sc.n, sc.dt, 1))
    print(f"engine.step_fused_tiled_multi host issue {e[0]:6.2f} us/call   wall {e[1]:6.2f} us/step")
    # the resident loop's fullest call: through a sea, with pose hold, applied wrench and recorder all set (one step, row 0)
    from silver2_isaacsim_amd.sea import SeaState
    eng.set_sea(SeaState.regular(0.4, 8.0, 0.0, current=(0.3, 0.0, 0.0))); eng.set_watch([0, 100, sc.n - 1])
    A, C = eng.alloc_tiled(6, sc.n), eng.alloc_tiled(nat.CTL_FIELDS, sc.n)
    L = torch.zeros((4, 13, 3), dtype=torch.float32, device=dev)
    g = bench(lambda: eng.step_fused_tiled_multi_sea(S, S2, sc.n, sc.dt, 1, 0, C, A, "body", log=L, every=1, phase=1, row0=0))
    print(f"engine.step_fused_tiled_multi_sea host issue {g[0]:6.2f} us/call   wall {g[1]:6.2f} us/step")
    eng.set_sea(None); eng.set_watch(None)
    # the plugin's call: 20 bodies on the simulator's tensors, prepared once, stream = the current one at each call
    m = 20
    eng20 = HydroEngine(m, dev, sc.rho, sc.g); eng20.set_params(sc.params[:m])
    st = torch.from_numpy(sc.state[:m]).to(dev)
    pos, ori, vel = st[:, 0:3].contiguous(), st[:, 3:7].contiguous(), st[:, 7:13].contiguous()
    aos = eng20.prepare_step_wrench_aos(pos, ori, vel)
    f = bench(lambda: aos(sc.dt))
    print(f"prepared step_wrench_aos (20) host issue {f[0]:6.2f} us/call   wall {f[1]:6.2f} us/step")
