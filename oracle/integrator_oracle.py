"""CPU oracle (NumPy, float64) for the device integrator: the closed-loop step of `hydro_integrate[_tiled]`,
`hydro_step_fused_tiled[_ke]` and `hydro_step_fused_tiled_multi` (`integrate_body<IMPLICIT>` in
silver2_isaacsim_amd/csrc/hydro_kernels.hip).

TEST INFRASTRUCTURE ONLY, like `hydro_oracle`.  The integrator is not part of the reference - PhysX integrates there
 - so this module restates this repository's own contract, `include/hydro.h` and DESIGN.md row (f-2):

  * linear: semi-implicit Euler, gravity along -z:      v' = v + dt (F / m - g e_z),   p' = p + dt v'
  * angular: box inertia I = m/12 (dy^2 + dz^2, dx^2 + dz^2, dx^2 + dy^2), body frame Euler equation
             I (w_b' - w_b) / dt = tau_b - w_b x I w_b,   w_b = R^T w,  tau_b = R^T tau,  w' = R w_b'
  * attitude: q' = normalise(q + dt/2 (w', 0) (x) q); R is the matrix of `hydro_oracle._rot_batch`, the quaternion used
             as given (a non-unit one included), as every kernel of the library does
  * implicit drag (`implicit_drag != 0` of the fused entries): the drag part of the wrench, k_lin v and k_ang w with
             k <= 0, is taken at the new velocity with the coefficients of the old state:
             v' = (m v + dt (F - k_lin v - m g e_z)) / (m - dt k_lin),   per principal axis likewise with I and k_ang.

`integrate` returns float64; the caller rounds to fp32 where the device stores fp32.  `integrator_error_ulps` is the
one per-field metric of the GPU tests and of the CPU test that shows the metric separates a wrong step from a right one
(tests/test_integrator_oracle.py): both use `STEP_ULP_BOUND`.
"""
from __future__ import annotations

import numpy as np

from . import hydro_oracle as ho

ULP = 2.0 ** -24
# Per-field bound of one device step against `integrate` (in units of ULP * the field's scale, see integrator_error_ulps):
# about 4x the largest value measured on the MI355X over every entry, coefficient format and size of
# tests/test_integrator_gpu.py: 6.06 (velocity, implicit form); the explicit form reached 3.64 (angular velocity).
STEP_ULP_BOUND = 24.0
GROUPS = ("position", "quaternion", "velocity", "angular_velocity")
_COEFF_COLS = slice(3, 10)          # cd_lin cd_ang damp_lin damp_ang lift am_lin am_ang


def box_inertia(params):
    """(N,3) principal moments of the box: m/12 (dy^2 + dz^2, dx^2 + dz^2, dx^2 + dy^2)."""
    p = np.asarray(params, dtype=np.float64)
    m, d2 = p[:, 10], p[:, 0:3] ** 2
    return (m / 12.0)[:, None] * np.stack([d2[:, 1] + d2[:, 2], d2[:, 0] + d2[:, 2], d2[:, 0] + d2[:, 1]], axis=1)


def _step(state, wrench, params, g, dt, k_lin=None, k_ang=None, mutate=()):
    """The step itself.  `mutate` names deliberate errors for the sensitivity test (tests/test_integrator_oracle.py);
    every caller outside that test uses `integrate`, i.e. no mutation."""
    s = np.asarray(state, dtype=np.float64)
    w6 = np.asarray(wrench, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    dt, g = float(dt), float(g)
    m = p[:, 10]
    implicit = k_lin is not None
    grav = np.zeros(3) if "no_gravity" in mutate else np.array([0.0, 0.0, -g])
    F, tau = w6[:, 0:3], w6[:, 3:6]
    v = s[:, 7:10]
    if implicit:
        kl = np.asarray(k_lin, dtype=np.float64)[:, None]
        den = (m[:, None] + dt * kl) if "den_plus" in mutate else (m[:, None] - dt * kl)
        gz = np.zeros(3) if "implicit_no_gravity" in mutate else grav
        v_new = (m[:, None] * v + dt * (F - kl * v + m[:, None] * gz)) / den
    else:
        v_new = v + dt * (F / m[:, None] + grav)
    pos = s[:, 0:3] + dt * (v if "old_velocity_position" in mutate else v_new)

    q = s[:, 3:7]
    R = ho._rot_batch(q)
    inertia = box_inertia(p)
    if "inertia_permuted" in mutate:
        inertia = inertia[:, [1, 2, 0]]
    to_body, to_world = ("nab,nb->na", "nba,nb->na") if "rotation_swapped" in mutate else ("nba,nb->na", "nab,nb->na")
    wb = np.einsum(to_body, R, s[:, 10:13])
    tb = np.einsum(to_body, R, tau)
    gyro = np.cross(wb, inertia * wb)
    if "no_gyro" in mutate:
        gyro = 0.0 * gyro
    elif "gyro_sign" in mutate:
        gyro = -gyro
    if implicit and "angular_explicit" not in mutate:
        ka = np.asarray(k_ang, dtype=np.float64)[:, None]
        nb = (inertia * wb + dt * (tb - ka * wb - gyro)) / (inertia - dt * ka)
    else:
        nb = wb + dt * (tb - gyro) / inertia
    w_new = np.einsum(to_world, R, nb)

    wq = nb if "body_omega_in_quaternion" in mutate else w_new
    qv, qw = q[:, 0:3], q[:, 3]
    dq = np.concatenate([wq * qw[:, None] + np.cross(wq, qv), -(wq * qv).sum(axis=1, keepdims=True)], axis=1)
    qn = q + 0.5 * dt * dq
    qn = qn / np.linalg.norm(qn, axis=1, keepdims=True)
    return np.concatenate([pos, qn, v_new, w_new], axis=1)


def integrate(state, wrench, params, g, dt, k_lin=None, k_ang=None):
    """One device step in fp64: (N,13) state and (N,6) [F | tau] world-frame wrench -> (N,13) float64.
    With k_lin / k_ang ((N,), the clamped drag coefficients of `drag_jacobian`) the implicit-drag form."""
    if (k_lin is None) != (k_ang is None):
        raise ValueError("k_lin and k_ang go together")
    return _step(state, wrench, params, g, dt, k_lin, k_ang)


def _coeffs(params, coeff_dtype):
    p = np.array(params, dtype=np.float64)
    if coeff_dtype == "f16":
        p[:, _COEFF_COLS] = p[:, _COEFF_COLS].astype(np.float16).astype(np.float64)
    elif coeff_dtype != "f32":
        raise ValueError("coeff_dtype must be 'f32' or 'f16'")
    return p


def drag_jacobian(state, params, comps, rho, coeff_dtype="f32"):
    """(k_lin, k_ang): the drag force / torque of the wrench is k_lin v / k_ang w, scaled by the safety clamp like the
    rest of it (hydro_body.h `assemble_wrench`):
        k_lin = -(1/2 rho |v| cd_lin A + damp_lin min(1, |v| / 0.2)) ratio scale
        k_ang = -(1/2 rho |w| cd_ang V + damp_ang min(1, |w| / 0.2)) ratio scale     (V: the volume, as the reference)
    `comps` is what hydro_oracle.solve_components / step_wrench return ('ratio', 'area' and, from step_wrench, 'scale';
    without 'scale' the clamp is taken as inactive).  coeff_dtype 'f16': the coefficients as the fp16 record holds them."""
    s = np.asarray(state, dtype=np.float64)
    p = _coeffs(params, coeff_dtype)
    speed = np.linalg.norm(s[:, 7:10], axis=1)
    wspeed = np.linalg.norm(s[:, 10:13], axis=1)
    vol = p[:, 0] * p[:, 1] * p[:, 2]
    ratio, area = comps["ratio"], comps["area"]
    scale = comps.get("scale", np.ones(len(s)))
    lin_quad = 0.5 * rho * speed * p[:, 3] * area
    ang_quad = np.where(wspeed > ho.SPEED_EPS, 0.5 * rho * wspeed * p[:, 4] * vol, 0.0)
    k_lin = -(lin_quad + p[:, 5] * np.minimum(1.0, speed / ho.LOW_SPEED_THRESHOLD)) * ratio * scale
    k_ang = -(ang_quad + p[:, 6] * np.minimum(1.0, wspeed / ho.LOW_SPEED_THRESHOLD)) * ratio * scale
    return k_lin, k_ang


def field_scales(state, wrench, params, g, dt, k=None, ref=None):
    """Per-body scales of the four field groups: the sum of the magnitudes of the terms that form each field, i.e. what
    fp32 rounding of the step is relative to.  Returns a dict of (N,3) (position, velocity: per component; angular
    velocity: per principal axis) and (N,) (quaternion) arrays.  `ref` (the fp64 result) adds |w'| to the angular scale:
    w' = R w_b' is a rotation of the new body-frame rate."""
    s = np.asarray(state, dtype=np.float64)
    w6 = np.asarray(wrench, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    dt, g = float(dt), float(g)
    m = p[:, 10][:, None]
    kl, ka = (np.zeros(len(s)), np.zeros(len(s))) if k is None else (np.abs(k[0]), np.abs(k[1]))
    kl, ka = kl[:, None], ka[:, None]
    gz = np.array([0.0, 0.0, g])
    av = np.abs(s[:, 7:10])
    sv = (m * av + dt * (np.abs(w6[:, 0:3]) + kl * av + m * gz)) / (m + dt * kl)
    sp = np.abs(s[:, 0:3]) + dt * sv
    inertia = box_inertia(p)
    wn = np.linalg.norm(s[:, 10:13], axis=1)[:, None]
    tn = np.linalg.norm(w6[:, 3:6], axis=1)[:, None]
    other = inertia[:, [1, 2, 0]] + inertia[:, [2, 0, 1]]            # I_b + I_c: the terms of (w_b x I w_b)_a
    sw = (inertia * wn + dt * (tn + ka * wn + wn * wn * other)) / (inertia + dt * ka)
    if ref is not None:
        sw = sw + np.linalg.norm(np.asarray(ref, dtype=np.float64)[:, 10:13], axis=1)[:, None]
    qn = np.linalg.norm(s[:, 3:7], axis=1)
    sq = qn * (1.0 + 0.5 * dt * np.linalg.norm(sw, axis=1))
    return {"position": sp, "quaternion": sq, "velocity": sv, "angular_velocity": sw}


def integrator_error_ulps(got, ref, state, wrench, params, g, dt, k=None, scales=None):
    """Per body and field group, |got - ref| / (ULP * scale) with the scales of `field_scales`: position and velocity
    per component, angular velocity per principal axis (the difference taken into the body frame of the input
    orientation), quaternion as a vector.  Returns {group: (N,) max over the group's components}.  k: (k_lin, k_ang) of
    the implicit form, None for the explicit one.  `scales` replaces the scales of this one step (a trajectory: the
    largest scales of the steps so far, see running_scales)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    sc = field_scales(state, wrench, params, g, dt, k, ref) if scales is None else scales
    d = got - ref
    q = np.asarray(state, dtype=np.float64)[:, 3:7]
    R = ho._rot_batch(q / np.linalg.norm(q, axis=1, keepdims=True))
    dw_b = np.einsum("nba,nb->na", R, d[:, 10:13])

    def ulps(diff, scale):
        # a field whose terms are all zero (a dry body at rest) must come out exactly: 0 / 0 is 0, x / 0 is inf;
        # NaN (a non-finite result) stays NaN
        diff = np.abs(diff)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(diff == 0.0, 0.0, diff / (ULP * scale))
    return {
        "position": ulps(d[:, 0:3], sc["position"]).max(axis=1),
        "quaternion": ulps(d[:, 3:7], sc["quaternion"][:, None]).max(axis=1),
        "velocity": ulps(d[:, 7:10], sc["velocity"]).max(axis=1),
        "angular_velocity": ulps(dw_b, sc["angular_velocity"]).max(axis=1),
    }


def running_scales(steps, params, g, dt):
    """For the per-step dicts of `closed_loop`: after step k, the largest field_scales of steps 1 .. k, per body and
    component.  A state carries the rounding of every step that made it - a body damped from 1 rad/s to 1e-6 rad/s in
    one step keeps the absolute error of the first one - so a trajectory is measured against the largest magnitudes its
    fields have had."""
    out, run = [], None
    for r in steps:
        sc = field_scales(r["input"], r["wrench"], params, g, dt, r["k"], r["state"])
        run = sc if run is None else {key: np.maximum(run[key], sc[key]) for key in sc}
        out.append(run)
    return out


def max_error_ulps(err):
    """Largest value over bodies and groups of an integrator_error_ulps result (NaN counts as infinite)."""
    return max(float(np.nan_to_num(e, nan=np.inf).max(initial=0.0)) for e in err.values())


def closed_loop(state, prev, params, rho, g, dt, steps, implicit=False, coeff_dtype="f32", semantics="numba"):
    """The fp64 closed loop the device runs: per step the oracle wrench (hydro_oracle.step_wrench, rounded to fp32 as
    the device hands it to its integrator), `integrate` (implicit: with drag_jacobian), the state rounded to fp32 as
    the device stores it; the previous velocity is the fp32 velocity of the step before.  Returns a list of per-step
    dicts: 'state' (the fp32 state after the step), 'input' (the state it started from), 'wrench', 'k', 'margin'
    (scenes.branch_margins of the input state).  tests/closed_loop_reference.py is this loop with the resident options as arguments."""
    from silver2_isaacsim_amd import scenes
    p = _coeffs(params, coeff_dtype)
    st = np.asarray(state, dtype=np.float32)
    pv = np.asarray(prev, dtype=np.float32)
    out = []
    for _ in range(steps):
        f, t, comps = ho.step_wrench(st, pv, p, rho, g, dt, semantics)
        wrench = np.concatenate([f, t], axis=1).astype(np.float32)
        k = drag_jacobian(st, p, comps, rho) if implicit else None
        new = integrate(st, wrench, p, g, dt, *(k if k is not None else (None, None)))
        out.append({"input": st, "wrench": wrench, "k": k, "margin": scenes.branch_margins(st, params),
                    "state": new.astype(np.float32)})
        pv, st = st[:, 7:13].copy(), out[-1]["state"]
    return out
