"""The fp64 closed loop of the resident steps, every option by argument: the one reference of the CPU tests that run a sea, a
seabed, mooring lines or tethers through steps (tests/test_sea.py, test_seabed.py, test_mooring.py, test_tether.py,
test_extremes.py, test_symmetry.py).  No device, no library.

With no option set it is `integrator_oracle.closed_loop` bit for bit (tests/test_closed_loop_reference.py); that one stays in
oracle/ - which may not import from tests/ - and carries `semantics` and 'margin' for the GPU tests.  A new resident option
adds an argument and a term HERE, in the kernel's order, not a copy of the loop.
"""
import numpy as np

from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io

import mooring_reference as mr
import sea_reference as sr
import seabed_reference as br
import tether_reference as tr


def closed_loop(state, prev, params, rho, g, dt, steps, *, sea=None, step0=0, applied=None, bed=None, moor=None, teth=None,
                implicit, coeff_dtype="f32", hydro=True):
    """Per step, in the order of `fused_step_in_registers`:
      1. the fp64 water of `sea` at the fp32 state, eta and u rounded to fp32 as the device holds them, and the fp32 RELATIVE
         state (sea_reference.water, .relative); without a sea the state itself
      2. hydro_oracle.step_wrench on the relative state
      3. the sum in fp64, left to right: hydro + `applied` ((n, 6), world frame) + the bed's wrench + the mooring lines'
         (`moor`: an (n, 9) record) + the tethers' (`teth`: an (n, 7) record), the last three of the TRUE state.  An absent
         term is not added: adding zeros would turn a -0.0 component into +0.0
      4. the sum rounded to fp32 once
      5. implicit: integrator_oracle.drag_jacobian from the relative state
      6. integrator_oracle.integrate on the true state
      7. the state rounded to fp32; the previous velocity is the fp32 velocity of the step before.
    hydro=False: a scene in which only the other terms act - the hydrodynamic wrench is zeros, there is no drag Jacobian, and
    the caller passes g = 0.

    Returns per-step dicts: 'input' (the fp32 state the step started from), 'state' (after it), 'wrench' (the fp32 sum),
    'hydro' (fp64), 'k' ((k_lin, k_ang) or None); with a sea 'eta', 'u' (fp32); with a bed 'bed' (its fp64 wrench), 'delta'
    ((n, 8) penetrations of the input state); with mooring 'line' (the fp64 wrench), 'tension', 'taut'; with tethers the same
    three as 'tether_line', 'tether_tension', 'tether_taut'."""
    p = io._coeffs(params, coeff_dtype)
    st = np.asarray(state, dtype=np.float32)
    pv = np.asarray(prev, dtype=np.float32)
    out = []
    for i in range(steps):
        r = {"input": st}
        s_rel, pv_rel = st, pv
        if sea is not None:
            eta, u = sr.water(sea, st[:, 0], st[:, 1], st[:, 2], step0 + i, dt)
            r["eta"], r["u"] = eta.astype(np.float32), u.astype(np.float32)
            s_rel, pv_rel = sr.relative(st, pv, r["eta"], r["u"])
        comps = None
        if hydro:
            f, t, comps = ho.step_wrench(s_rel, pv_rel, p, rho, g, dt)
            r["hydro"] = np.concatenate([f, t], axis=1).astype(np.float64)
        else:
            r["hydro"] = np.zeros((len(st), 6))
        total = r["hydro"]
        if applied is not None:
            total = total + np.asarray(applied, np.float64)
        if bed is not None:
            r["bed"], r["delta"] = br.wrench(bed, st, params), br.penetration(bed, st, params)
            total = total + r["bed"]
        if moor is not None:
            r["line"], r["tension"], r["taut"] = mr.wrench(moor, st), mr.tension(moor, st), mr.taut(moor, st)
            total = total + r["line"]
        if teth is not None:
            r["tether_line"], r["tether_tension"], r["tether_taut"] = tr.wrench(teth, st), tr.tension(teth, st), tr.taut(teth, st)
            total = total + r["tether_line"]
        r["wrench"] = total.astype(np.float32)
        r["k"] = io.drag_jacobian(s_rel, p, comps, rho) if (implicit and hydro) else None
        new = io.integrate(st, r["wrench"], p, g, dt, *(r["k"] if r["k"] is not None else (None, None)))
        r["state"] = new.astype(np.float32)
        out.append(r)
        pv, st = st[:, 7:13].copy(), r["state"]
    return out
