#!/usr/bin/env python3
"""Generate tests/golden/warp_reference.npz by EXECUTING THE REFERENCE'S WARP CALCULATOR under a stand-in for Warp.

Needs a checkout of the reference (the path below), like make_golden.py; the fixture it writes is committed, the
reference never travels.  Usage:

    python3 -B tests/golden/make_golden_warp.py

A script of its own because make_golden.py gives `warp` an empty import shell; here `warp` is tests/tools/warp_standin.py
(float64, Warp's zero-initialised locals modelled, see its docstring), installed BEFORE make_golden.py is imported for its
harness, so that the reference's `hydrodynamics_behavior.py` imports its real `warp_hydrodynamics_wrapper.py` (unchanged:
keypoint order, face tables, parameter vector, added-mass vectors, graph capture and replay) and that one the kernel file
`warp_hydrodynamics.py`, loaded through the stand-in's `ast` pass.  Nothing is written into the reference tree.

Per body of tests/populations.py `warp_reference_populations()` (inputs are not stored, a digest of each population is):
  with quat_rotate = "matrix"  the wrapper's eight outputs and the net force / torque that the reference's own
                               `_apply_behavior` hands to the simulator with that wrapper as its calculator (the harness of
                               make_golden.py: in-memory view, float64 CPU tensors, mass from the parameters);
  with quat_rotate = "warp"    that net wrench again (Warp's own polynomial definition of quat_rotate);
  flags   finite     every stored number of both runs is finite
          hole       a zero-initialised local mattered in either run: the function that falls off its end at
                     speed <= 1e-6 (N1) or the lift direction that is read unassigned (N4)
          unit       | |q| - 1 | <= 1e-6
          margin_ok  scenes.branch_margins >= 1e-4
  formula_effect     hydro_oracle.wrench_error between the two net wrenches.
"""
from __future__ import annotations

import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "tools"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import warp_standin  # noqa: E402

REFERENCE_SCRIPTS = "/root/reference/src/scripts"
FIXTURE = os.path.join(HERE, "warp_reference.npz")


def import_reference():
    """(make_golden module with the reference's behaviour imported against the stand-in, the reference's Warp wrapper module)."""
    warp_standin.install()
    kernels = warp_standin.load_kernel_module(os.path.join(REFERENCE_SCRIPTS, "physics", "warp_hydrodynamics.py"),
                                              "physics.warp_hydrodynamics")
    holes = {k: v for k, v in kernels.__wp_rewritten__.items() if any(v)}
    print("zero-initialisation rewritten in (local read, fall off the end):", holes)
    assert sum(a for a, _ in holes.values()) == 1 and sum(b for _, b in holes.values()) == 1, "N1 and N4 are one function each"
    import make_golden as mg                                        # puts the reference on sys.path, shells for Kit
    import physics.warp_hydrodynamics_wrapper as ref_w
    assert ref_w.solve_hydrodynamics_kernel is kernels.solve_hydrodynamics_kernel
    assert mg.REF_B.WarpHydrodynamicsWrapper is ref_w.WarpHydrodynamicsWrapper
    return mg, ref_w


class _Recording:
    """The reference's Warp wrapper as the behaviour's calculator; keeps a copy of the eight tensors it returned."""

    def __init__(self, wrapper):
        self.wrapper, self.last = wrapper, None

    def calculate_hydrodynamic_forces(self, *args):
        out = self.wrapper.calculate_hydrodynamic_forces(*args)
        self.last = np.stack([o[0].numpy().copy() for o in out])
        return out


def reference_body(mg, ref_w, state, prev, params, rho, g, dt):
    """One body through the reference's `_apply_behavior` with its executed Warp wrapper -> (components (8,3), net force,
    net torque, a zero-initialised local mattered)."""
    import torch
    f64 = lambda x: torch.tensor(np.asarray(x, dtype=np.float64)[None, :])   # noqa: E731
    s = np.asarray(state, dtype=np.float64)
    dims = [float(x) for x in params[0:3]]
    cd_lin, cd_ang, damp_lin, damp_ang, lift_c, am_lin, am_ang = (float(x) for x in params[3:10])
    events = len(warp_standin.EVENTS)
    obj = object.__new__(mg.REF_B.HydrodynamicsBehavior)
    obj._device = "cpu"
    obj._rigid_prim_view = mg._View(f64(s[0:3]), f64(s[[6, 3, 4, 5]]), f64(s[7:13]))      # simulator order: wxyz
    obj._hydro_calculator = _Recording(ref_w.WarpHydrodynamicsWrapper(
        dims[0], dims[1], dims[2], cd_lin, cd_ang, damp_lin, damp_ang, float(rho), float(g), am_lin, am_ang, lift_c, device="cpu"))
    obj._mass = torch.tensor(float(params[10]), dtype=torch.float64)
    obj._last_linear_velocity = f64(prev[0:3])
    obj._last_angular_velocity = f64(prev[3:6])
    obj._apply_behavior(float(dt))
    f, t = obj._rigid_prim_view.applied
    return obj._hydro_calculator.last, f[0].numpy(), t[0].numpy(), len(warp_standin.EVENTS) > events


def reference_population(mg, ref_w, pop):
    from oracle import hydro_oracle as ho
    from silver2_isaacsim_amd import scenes
    state, prev, params, rho, g, dt = pop
    n = len(state)
    comps, hole = np.zeros((n, 8, 3)), np.zeros(n, dtype=bool)
    net = {m: (np.zeros((n, 3)), np.zeros((n, 3))) for m in warp_standin.QUAT_ROTATE_MODES}
    with np.errstate(all="ignore"):
        for mode in warp_standin.QUAT_ROTATE_MODES:
            warp_standin.set_quat_rotate(mode)
            for i in range(n):
                c, net[mode][0][i], net[mode][1][i], fired = reference_body(mg, ref_w, state[i], prev[i], params[i], rho, g, dt)
                hole[i] |= fired
                if mode == "matrix":
                    comps[i] = c
        warp_standin.set_quat_rotate("matrix")
        (nf, nt), (wf, wt) = net["matrix"], net["warp"]
        finite = np.isfinite(np.concatenate([comps.reshape(n, -1), nf, nt, wf, wt], axis=1)).all(axis=1)
        q = state[:, 3:7].astype(np.float64)
        unit = np.abs(np.linalg.norm(q, axis=1) - 1.0) <= 1e-6
        margin_ok = scenes.branch_margins(state, params) >= 1e-4
        effect = ho.wrench_error(wf, wt, nf, nt, params, rho, g)
    return {"components": comps, "net_force": nf, "net_torque": nt, "net_force_warp": wf, "net_torque_warp": wt,
            "finite": finite, "hole": hole, "unit": unit, "margin_ok": margin_ok, "formula_effect": effect}


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, value in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(value), allow_pickle=False)


def main():
    import populations
    import reference_fuzz as rf
    mg, ref_w = import_reference()
    arrays = {}
    for name, pop in populations.warp_reference_populations().items():
        out = reference_population(mg, ref_w, pop)
        arrays[f"{name}_sha256"] = np.array(rf.population_digest(*pop[:3]))
        for k, v in out.items():
            arrays[f"{name}_{k}"] = v
        ok = out["finite"] & ~out["hole"]
        sel = ok & out["unit"] & out["margin_ok"]
        kinds = sorted({e[:2] for e in warp_standin.EVENTS})
        print(f"{name}: {len(out['hole'])} bodies, finite {int(out['finite'].sum())}, hole {int(out['hole'].sum())}, "
              f"unit {int(out['unit'].sum())}, margin_ok {int(out['margin_ok'].sum())}; formula_effect max over "
              f"unit & margin_ok & finite & ~hole ({int(sel.sum())}): {out['formula_effect'][sel].max(initial=0.0):.3e}, "
              f"over finite & ~hole & unit: {out['formula_effect'][ok & out['unit']].max(initial=0.0):.3e}; events so far {kinds}")
    save_npz(FIXTURE, arrays)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} B")


if __name__ == "__main__":
    main()
