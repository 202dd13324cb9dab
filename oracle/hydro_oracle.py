"""CPU oracle (NumPy, float64) for the per-body hydrodynamic wrench path.

TEST INFRASTRUCTURE ONLY.  Nothing in the product package
(`silver2_isaacsim_amd/`) may import this module; only `tests/`,
`__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg use it, and
only as the checker.

This is a restatement, in this repo's own code, of the reference algorithm:

  * kernels      /root/reference/src/scripts/physics/numba_hydrodynamics.py:9-314
  * geometry     /root/reference/src/scripts/physics/numba_hydrodynamics_wrapper.py:55-112
  * epilogue     /root/reference/src/scripts/physics/hydrodynamics_behavior.py:194-238

Parity pinning: `tests/golden/make_golden.py` executes the reference's own
functions (identity-`njit` stub; Numba itself is not installed in the build
container) on seeded inputs and commits inputs+outputs as `.npz` fixtures;
`tests/test_oracle_golden.py` checks this module against them to <=1e-12.
The behaviour-level epilogue (A13-A16) is pinned the same way: the generator
executes the reference's own `_apply_behavior` (hydrodynamics_behavior.py:176-238,
float64 torch tensors, Kit-only imports replaced by empty shells) and stores the
net force / torque it hands to the simulator; the survey's K1-K5 known-answer
vectors are checked too.  Only the C1 trajectory's
integrator (PhysX in the reference) is this repo's own.

Documented completion: the reference's
`calculate_pressure_and_area` has no return value when `speed <= 1e-6`
(numba_hydrodynamics.py:118,143).  The evident intent - the "Defaults" at
:113-115 - is `(center_of_buoyancy, 0.0)`; this oracle, the golden generator
and the HIP kernels all apply that completion.

Warp twin (`semantics="warp"`): the places where warp_hydrodynamics.py:233-335 differs from the Numba
path (added-mass rotation, centres of a dry body, centre of buoyancy when the top keypoints are exactly
on the surface) are restated here.  Pinned the same way as the Numba mode:
`tests/golden/make_golden_warp.py` executes the reference's Warp source and its wrapper under a stand-in
for the Warp runtime (`tests/tools/warp_standin.py`: float64, Warp's zero-initialised locals modelled,
`quat_rotate` bound to the matrix form) through the reference's `_apply_behavior`, and
`tests/test_warp_semantics.py` holds this module to those outputs at 1e-9.  Not pinned: NVIDIA's runtime
and its fp32 rounding.  Warp's own `quat_rotate(q, v)` equals R(q) v + 2 (|q|^2 - 1) v; this module and
the kernels use R(q) v in both modes (up to 1.0e-5 of the wrench on fp32-rounded unit
quaternions, order one on non-unit ones).  The Numba mode is unaffected.

Field orders used everywhere in this repo
  state  (13): px py pz | qx qy qz qw | vx vy vz | wx wy wz     (quat xyzw)
  prev    (6): vx vy vz | wx wy wz      (velocity at the previous step)
  params (11): dimx dimy dimz | cd_lin cd_ang | damp_lin damp_ang | lift |
               am_lin am_ang | mass
"""
from __future__ import annotations

import numpy as np

STATE_FIELDS = ("px", "py", "pz", "qx", "qy", "qz", "qw",
                "vx", "vy", "vz", "wx", "wy", "wz")
PREV_FIELDS = ("pvx", "pvy", "pvz", "pwx", "pwy", "pwz")
PARAM_FIELDS = ("dimx", "dimy", "dimz", "cd_lin", "cd_ang", "damp_lin",
                "damp_ang", "lift", "am_lin", "am_ang", "mass")
COMPONENT_FIELDS = ("buoyancy_force", "drag_force", "lift_force", "drag_torque",
                    "added_mass_force", "added_mass_torque",
                    "center_of_buoyancy", "center_of_pressure")

LOW_SPEED_THRESHOLD = 0.2     # numba_hydrodynamics.py:154
SPEED_EPS = 1e-6              # :118,156,170,192,286
DRY_EPS = 1e-9                # :192,225,277
AREA_EPS = 1e-6               # :140
HEIGHT_EPS = 1e-6             # :92
AXIS_EPS = 1e-6               # :210
MAX_ACCEL = 500.0             # hydrodynamics_behavior.py:221
CLAMP_EPS = 1e-6              # hydrodynamics_behavior.py:224

# bits of aux['branches']: every decision of the model (solve_components, step_wrench), so that two evaluations can be
# compared decision by decision: 27 wet keypoints (lattice order), moving, spinning, the six faces' `take` (+X -X +Y
# -Y +Z -Z), has_area, lift_ok, wet (ratio > 1e-9), partially submerged, clamp active (scale < 1)
BRANCH_NAMES = (tuple(f"wet_keypoint_{k}" for k in range(27)) + ("moving", "spinning")
                + tuple(f"take_{f}" for f in ("+x", "-x", "+y", "-y", "+z", "-z"))
                + ("has_area", "lift_ok", "live", "partial", "clamp"))
BRANCH_CLAMP = BRANCH_NAMES.index("clamp")


# --------------------------------------------------------------------------
# geometry (numba_hydrodynamics_wrapper.py:55-112)
# --------------------------------------------------------------------------
def lattice_keypoints(dims):
    """27 body-frame keypoints {-hx,0,hx} x {-hy,0,hy} x {-hz,0,hz} (wrapper :55-73)."""
    hx, hy, hz = (0.5 * float(d) for d in dims)
    # the middle coordinates are the literal 0 of the wrapper's table, not 0 * h: a NaN or infinite dimension stays out of them
    pts = [(i * hx if i else 0.0, j * hy if j else 0.0, k * hz if k else 0.0)
           for k in (1, 0, -1) for j in (1, 0, -1) for i in (-1, 0, 1)]
    return np.asarray(pts, dtype=np.float64)


def box_faces(dims):
    """Face centres, outward normals and areas of the box (wrapper :75-99).

    Face order: +X, -X, +Y, -Y, +Z, -Z.
    """
    w, d, h = (float(x) for x in dims)
    normals = np.zeros((6, 3))
    centers = np.zeros((6, 3))
    half = (0.5 * w, 0.5 * d, 0.5 * h)
    for axis in range(3):
        for s, sign in enumerate((1.0, -1.0)):
            normals[2 * axis + s, axis] = sign
            centers[2 * axis + s, axis] = sign * half[axis]
    areas = np.array([d * h, d * h, w * h, w * h, w * d, w * d], dtype=np.float64)
    return centers, normals, areas


def added_mass_diagonal(dims, rho, am_lin, am_ang):
    """Diagonal of the 6x6 added-mass matrix (wrapper :101-112)."""
    w, d, h = (float(x) for x in dims)
    vol = w * d * h
    lin = vol * am_lin * rho
    return np.array([lin, lin, lin,
                     vol * (d * d + h * h) * am_ang * rho,
                     vol * (w * w + h * h) * am_ang * rho,
                     vol * (w * w + d * d) * am_ang * rho], dtype=np.float64)


# --------------------------------------------------------------------------
# scalar (one body) restatement - follows the reference step by step
# --------------------------------------------------------------------------
def rotation_from_quat_xyzw(q):
    """Unit quaternion [x,y,z,w] -> row-major 3x3, no normalisation
    (numba_hydrodynamics.py:9-51)."""
    x, y, z, w = (float(c) for c in q)
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz = x * x2, x * y2, x * z2
    yy, yz, zz = y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    return np.array([[1.0 - (yy + zz), xy - wz, xz + wy],
                     [xy + wz, 1.0 - (xx + zz), yz - wx],
                     [xz - wy, yz + wx, 1.0 - (xx + yy)]], dtype=np.float64)


def submersion_and_cob(world_pts, position, semantics="numba"):
    """Submersion ratio from the z-extent, CoB = mean of points with z<0
    (numba_hydrodynamics.py:54-105).  semantics="warp": no early return for a body that is fully in by bounds - its
    CoB is the mean of whatever points are wet (warp_hydrodynamics.py:58-61), which differs from the position only when
    the top keypoint is exactly on the surface (z = 0 is not wet)."""
    z = world_pts[:, 2]
    # `if pz < z_min: z_min = pz` from +inf (:62-77): a NaN height never enters, and with nothing but NaNs z_min stays +inf (dry)
    z_lo = float(np.where(np.isnan(z), np.inf, z).min())
    z_hi = float(np.where(np.isnan(z), -np.inf, z).max())
    if z_lo >= 0.0:
        return 0.0, position.copy()
    if z_hi <= 0.0:
        wet = z < 0.0
        if semantics == "warp" and 0 < int(wet.sum()) < len(z):     # all 27 wet: the mean IS the position
            return 1.0, world_pts[wet].sum(axis=0) / int(wet.sum())
        return 1.0, position.copy()
    height = z_hi - z_lo
    if height < HEIGHT_EPS:
        ratio = 1.0 if z_lo < 0.0 else 0.0
    else:
        with np.errstate(invalid="ignore"):
            ratio = -z_lo / height                                       # (Inf / Inf = NaN stays: `if ratio > 1.0` is false)
        if ratio > 1.0:
            ratio = 1.0
    wet = z < 0.0
    n_wet = int(wet.sum())
    cob = position.copy() if n_wet == 0 else world_pts[wet].sum(axis=0) / n_wet
    return ratio, cob


def pressure_centre_and_area(speed, vel_dir, cob, rot, position, dims):
    """Projected area of the wet faces whose normal opposes the velocity and the
    area-weighted centre of those faces (numba_hydrodynamics.py:108-143).
    `speed <= 1e-6` -> (cob, 0.0): the N1 completion, see module docstring."""
    if not speed > SPEED_EPS:
        return cob.copy(), 0.0
    centers, normals, areas = box_faces(dims)
    area = 0.0
    weighted = np.zeros(3)
    for f in range(6):
        n_w = rot @ normals[f]
        c_w = rot @ centers[f] + position
        alignment = -float(n_w @ vel_dir)
        if alignment > 0.0 and c_w[2] < 0.0:
            a = alignment * areas[f]
            area += a
            weighted += c_w * a
    cop = weighted / area if area > AREA_EPS else cob.copy()
    return cop, area


def hybrid_drag(speed, vel_dir, ratio, rho, area, volume,
                cd_lin, damp_lin, v, cd_ang, damp_ang, w):
    """Quadratic + linear drag force and torque (numba_hydrodynamics.py:146-182)."""
    quad_f = np.zeros(3)
    if speed > SPEED_EPS:
        quad_f = -(0.5 * rho * speed ** 2 * cd_lin * area) * vel_dir
    s_lin = speed / LOW_SPEED_THRESHOLD if speed < LOW_SPEED_THRESHOLD else 1.0
    force = (quad_f - damp_lin * v * s_lin) * ratio

    w_speed = float(np.linalg.norm(w))
    quad_t = np.zeros(3)
    if w_speed > SPEED_EPS:
        quad_t = -(0.5 * rho * w_speed ** 2 * cd_ang * volume) * (w / w_speed)
    s_ang = w_speed / LOW_SPEED_THRESHOLD if w_speed < LOW_SPEED_THRESHOLD else 1.0
    torque = (quad_t - damp_ang * w * s_ang) * ratio
    return force, torque


def lift_force(speed, vel_dir, rot, area, rho, lift_coeff, ratio):
    """Flat-plate angle-of-attack lift (numba_hydrodynamics.py:185-217)."""
    if speed < SPEED_EPS or ratio <= DRY_EPS:
        return np.zeros(3)
    up = rot[:, 2]
    d = -float(up @ vel_dir)
    d = max(-1.0, min(1.0, d))
    c_l = np.sin(2.0 * np.arcsin(d))
    mag = 0.5 * rho * speed ** 2 * c_l * area * lift_coeff
    axis = np.cross(vel_dir, up)
    n_axis = float(np.linalg.norm(axis))
    if n_axis < AXIS_EPS:
        return np.zeros(3)
    direction = np.cross(axis / n_axis, vel_dir)
    return mag * direction * ratio


def added_mass(ratio, a, alpha, rot, diag, semantics="numba"):
    """-M * body-frame acceleration, rotated back (numba_hydrodynamics.py:220-253).
    semantics="warp": the Warp twin rotates the world accelerations with quat_rotate(q, .) = R
    instead of R^T (warp_hydrodynamics.py:216-217); everything else is the same."""
    if ratio <= DRY_EPS:
        return np.zeros(3), np.zeros(3)
    to_local = rot if semantics == "warp" else rot.T
    a_b = to_local @ a
    al_b = to_local @ alpha
    f_b = -diag[:3] * a_b
    t_b = -diag[3:] * al_b
    return (rot @ f_b) * ratio, (rot @ t_b) * ratio


def solve_components_one(p, q, v, w, a, alpha, params, rho, g, semantics="numba"):
    """One body, 9 outputs in the reference's order
    (numba_hydrodynamics.py:256-314).  `params` = the 11 PARAM_FIELDS.
    semantics="warp": warp_hydrodynamics.py:233-335 where it differs (added mass, N3; a dry body
    reports cob = cop = centre of its wet keypoints or its position, N6)."""
    p, q, v, w, a, alpha = (np.asarray(x, dtype=np.float64) for x in (p, q, v, w, a, alpha))
    dims = np.asarray(params[:3], dtype=np.float64)
    cd_lin, cd_ang, damp_lin, damp_ang, lift_c, am_lin, am_ang = (float(x) for x in params[3:10])
    volume = float(dims[0] * dims[1] * dims[2])

    rot = rotation_from_quat_xyzw(q)
    world = lattice_keypoints(dims) @ rot.T + p
    ratio, cob = submersion_and_cob(world, p, semantics)
    if ratio <= DRY_EPS:
        z3 = np.zeros(3)
        if semantics == "warp":                # warp_hydrodynamics.py:58-61,283-290: outputs initialised, cop = cob
            return tuple(z3.copy() for _ in range(6)) + (cob.copy(), cob.copy(), 0.0)
        return tuple(z3.copy() for _ in range(8)) + (0.0,)

    buoy = np.array([0.0, 0.0, rho * (ratio * volume) * g])
    speed = float(np.linalg.norm(v))
    vel_dir = v / speed if speed > SPEED_EPS else np.zeros(3)
    cop, area = pressure_centre_and_area(speed, vel_dir, cob, rot, p, dims)
    drag_f, drag_t = hybrid_drag(speed, vel_dir, ratio, rho, area, volume,
                                 cd_lin, damp_lin, v, cd_ang, damp_ang, w)
    lift_f = lift_force(speed, vel_dir, rot, area, rho, lift_c, ratio)
    am_f, am_t = added_mass(ratio, a, alpha, rot,
                            added_mass_diagonal(dims, rho, am_lin, am_ang), semantics)
    return buoy, drag_f, lift_f, drag_t, am_f, am_t, cob, cop, ratio


def behavior_epilogue_one(p, comps, mass):
    """Lever-arm torques, sum and the 500 m/s^2 * mass clamp
    (hydrodynamics_behavior.py:212-226), float64."""
    buoy, drag_f, lift_f, drag_t, am_f, am_t, cob, cop = comps[:8]
    p = np.asarray(p, dtype=np.float64)
    t_b = np.cross(cob - p, buoy)
    t_d = np.cross(cop - p, drag_f)
    t_l = np.cross(cop - p, lift_f)
    net_f = buoy + drag_f + lift_f + am_f
    net_t = t_b + t_d + t_l + drag_t + am_t
    scale = min(1.0, float(mass) * MAX_ACCEL / (float(np.linalg.norm(net_f)) + CLAMP_EPS))
    return net_f * scale, net_t * scale, scale


# --------------------------------------------------------------------------
# vectorised batch versions (same arithmetic, N bodies at once)
# --------------------------------------------------------------------------
def _rot_batch(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz = x * x2, x * y2, x * z2
    yy, yz, zz = y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    r = np.empty((q.shape[0], 3, 3), dtype=np.result_type(q.dtype, np.float64))
    r[:, 0, 0] = 1.0 - (yy + zz); r[:, 0, 1] = xy - wz;         r[:, 0, 2] = xz + wy
    r[:, 1, 0] = xy + wz;         r[:, 1, 1] = 1.0 - (xx + zz); r[:, 1, 2] = yz - wx
    r[:, 2, 0] = xz - wy;         r[:, 2, 1] = yz + wx;         r[:, 2, 2] = 1.0 - (xx + yy)
    return r


_LATTICE_IJK = np.array([(i, j, k) for k in (1, 0, -1) for j in (1, 0, -1) for i in (-1, 0, 1)],
                        dtype=np.float64)  # (27,3)


def _f32(x):
    """x rounded to fp32 and back to the type it had (the mutants of `solve_components`)."""
    return np.asarray(x).astype(np.float32).astype(np.asarray(x).dtype)


# Deliberate fp32 steps for tests/test_wrench_metric.py, which shows that `wrench_error_ulps` catches them; every
# other caller leaves `mutate` empty.
MUTATIONS = ("rotation_f32", "heights_f32", "inv_speed_seed")


def solve_components(state, accel, params, rho, g, semantics="numba", dtype=np.float64, mutate=()):
    """Vectorised A1-A11 (semantics as in `solve_components_one`).

    state  (N,13), accel (N,6) [a | alpha], params (N,11), evaluated in `dtype`: float64 (default), or np.longdouble
    for the high-precision reference of `wrench_error_ulps` (the same operations, x87 80-bit where numpy has it).
    Returns dict with the eight (N,3) COMPONENT_FIELDS plus 'ratio' (N,) and
    diagnostic 'area' (N,), 'rest' (N,) bool = N1 completion fired, 'branches' (N,) int64 = BRANCH_BITS of the
    decisions taken (see `branch_flips`).
    `mutate` (names from MUTATIONS): the rotation matrix rounded to fp32, the keypoint heights rounded to fp32, or
    1/|v| taken from the fp32 reciprocal of the fp32 speed (a hardware seed without its Newton step).
    """
    if not set(mutate) <= set(MUTATIONS):
        raise ValueError(f"unknown mutation in {mutate}")
    state = np.asarray(state, dtype=dtype)
    accel = np.asarray(accel, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    n = state.shape[0]
    p, q, v, w = state[:, 0:3], state[:, 3:7], state[:, 7:10], state[:, 10:13]
    a, alpha = accel[:, 0:3], accel[:, 3:6]
    dims = params[:, 0:3]
    cd_lin, cd_ang, damp_lin, damp_ang, lift_c, am_lin, am_ang = (params[:, i] for i in range(3, 10))
    half = 0.5 * dims
    volume = dims[:, 0] * dims[:, 1] * dims[:, 2]
    rot = _rot_batch(q)
    if "rotation_f32" in mutate:
        rot = _f32(rot)

    # A2/A3: world keypoints, extent ratio, CoB
    # (the middle coordinates are the literal 0 of the wrapper's table, not 0 * h: a NaN or infinite dimension stays out of them)
    local = np.where(_LATTICE_IJK[None, :, :] == 0.0, 0.0, _LATTICE_IJK[None, :, :] * half[:, None, :])          # (N,27,3)
    # R k summed in the order written, x then y then z, as any sequential evaluation of the reference's source does:
    # einsum's order is numpy's choice, and a body within 1e-8 of the dry threshold sees one ulp of a keypoint height
    world = (rot[:, None, :, 0] * local[:, :, None, 0] + rot[:, None, :, 1] * local[:, :, None, 1]
             + rot[:, None, :, 2] * local[:, :, None, 2]) + p[:, None, :]                      # (N,27,3)
    if "heights_f32" in mutate:
        world[:, :, 2] = _f32(world[:, :, 2])
    z = world[:, :, 2]
    # `if pz < z_min: z_min = pz` from +inf (:62-77): a NaN height never enters; with nothing but NaNs z_min stays +inf (dry)
    z_lo, z_hi = np.where(np.isnan(z), np.inf, z).min(axis=1), np.where(np.isnan(z), -np.inf, z).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        height = z_hi - z_lo
        frac = -z_lo / height
        frac = np.where(frac > 1.0, 1.0, frac)                          # `if ratio > 1.0: ratio = 1.0`: a NaN (Inf / Inf) stays
    frac = np.where(height < HEIGHT_EPS, np.where(z_lo < 0.0, 1.0, 0.0), frac)
    ratio = np.where(z_lo >= 0.0, 0.0, np.where(z_hi <= 0.0, 1.0, frac))
    wet = z < 0.0
    n_wet = wet.sum(axis=1)
    partial = (z_lo < 0.0) & (z_hi > 0.0) & (n_wet > 0)
    mean_wet = np.where(wet[:, :, None], world, 0.0).sum(axis=1) / np.maximum(n_wet, 1)[:, None]
    # Warp twin: the mean of the wet points whenever there are any (warp_hydrodynamics.py:58-61), also for a body whose
    # top keypoint is exactly on the surface; with all 27 wet the mean is the position itself
    use_mean = (partial | ((n_wet > 0) & (n_wet < 27))) if semantics == "warp" else partial
    cob = np.where(use_mean[:, None], mean_wet, p)

    live = ~(ratio <= DRY_EPS)                                           # `if sub_ratio <= 1e-9: return zeros` (:277): a NaN ratio is not dry

    # A5
    buoy = np.zeros((n, 3), dtype=dtype)
    buoy[:, 2] = rho * (ratio * volume) * g

    # A6
    speed = np.linalg.norm(v, axis=1)
    moving = speed > SPEED_EPS
    if "inv_speed_seed" in mutate:
        inv = _f32(1.0 / _f32(np.where(moving, speed, 1.0)))
        vel_dir = np.where(moving[:, None], v * inv[:, None], 0.0)
    else:
        vel_dir = np.where(moving[:, None], v / np.where(moving, speed, 1.0)[:, None], 0.0)

    # A7 (N1 completion when not moving)
    area = np.zeros(n, dtype=dtype)
    weighted = np.zeros((n, 3), dtype=dtype)
    takes = []
    face_area = np.stack([dims[:, 1] * dims[:, 2], dims[:, 0] * dims[:, 2], dims[:, 0] * dims[:, 1]], axis=1)
    for axis in range(3):
        for sign in (1.0, -1.0):
            n_w = sign * rot[:, :, axis]
            c_w = sign * half[:, axis, None] * rot[:, :, axis] + p
            alignment = -np.einsum("na,na->n", n_w, vel_dir)
            take = moving & (alignment > 0.0) & (c_w[:, 2] < 0.0)
            takes.append(take)
            a_f = np.where(take, alignment * face_area[:, axis], 0.0)
            area += a_f
            weighted += np.where(take[:, None], c_w * a_f[:, None], 0.0)     # (a face that is not taken adds nothing, whatever its centre)
    has_area = area > AREA_EPS
    cop = np.where(has_area[:, None], weighted / np.where(has_area, area, 1.0)[:, None], cob)

    # A8
    quad_f = -(0.5 * rho * speed ** 2 * cd_lin * area)[:, None] * vel_dir
    s_lin = np.where(speed < LOW_SPEED_THRESHOLD, speed / LOW_SPEED_THRESHOLD, 1.0)
    drag_f = (quad_f - (damp_lin * s_lin)[:, None] * v) * ratio[:, None]
    w_speed = np.linalg.norm(w, axis=1)
    spinning = w_speed > SPEED_EPS
    w_dir = np.where(spinning[:, None], w / np.where(spinning, w_speed, 1.0)[:, None], 0.0)
    quad_t = -(0.5 * rho * w_speed ** 2 * cd_ang * volume)[:, None] * w_dir
    s_ang = np.where(w_speed < LOW_SPEED_THRESHOLD, w_speed / LOW_SPEED_THRESHOLD, 1.0)
    drag_t = (quad_t - (damp_ang * s_ang)[:, None] * w) * ratio[:, None]

    # A9
    up = rot[:, :, 2]
    d = np.clip(-np.einsum("na,na->n", up, vel_dir), -1.0, 1.0)
    c_l = np.sin(2.0 * np.arcsin(d))
    mag = 0.5 * rho * speed ** 2 * c_l * area * lift_c
    axis_v = np.cross(vel_dir, up)
    n_axis = np.linalg.norm(axis_v, axis=1)
    lift_ok = (~(speed < SPEED_EPS)) & (~(n_axis < AXIS_EPS))
    direction = np.cross(axis_v / np.where(lift_ok, n_axis, 1.0)[:, None], vel_dir)
    lift_f = np.where(lift_ok[:, None], (mag * ratio)[:, None] * direction, 0.0)

    # A10
    lin = volume * am_lin * rho
    m_ang = np.stack([volume * (dims[:, 1] ** 2 + dims[:, 2] ** 2) * am_ang * rho,
                      volume * (dims[:, 0] ** 2 + dims[:, 2] ** 2) * am_ang * rho,
                      volume * (dims[:, 0] ** 2 + dims[:, 1] ** 2) * am_ang * rho], axis=1)
    to_local = "nab,nb->na" if semantics == "warp" else "nba,nb->na"     # N3: R (Warp) / R^T (Numba)
    a_b = np.einsum(to_local, rot, a)
    al_b = np.einsum(to_local, rot, alpha)
    am_f = np.einsum("nab,nb->na", rot, -lin[:, None] * a_b) * ratio[:, None]
    am_t = np.einsum("nab,nb->na", rot, -m_ang * al_b) * ratio[:, None]

    out = {
        "buoyancy_force": buoy, "drag_force": drag_f, "lift_force": lift_f,
        "drag_torque": drag_t, "added_mass_force": am_f, "added_mass_torque": am_t,
        "center_of_buoyancy": cob, "center_of_pressure": cop,
    }
    for k in out:                       # A4: dry bodies return zeros for everything
        if semantics == "warp" and k in ("center_of_buoyancy", "center_of_pressure"):
            # N6: cob as computed (position, or mean of the wet keypoints), cop = cob
            out[k] = np.where(live[:, None], out[k], cob)
            continue
        out[k] = np.where(live[:, None], out[k], 0.0)
    out["ratio"] = np.where(live, ratio, 0.0)
    out["area"] = np.where(live, area, 0.0)
    out["rest"] = live & ~moving
    flags = [wet[:, k] for k in range(27)] + [moving, spinning] + takes + [has_area, lift_ok, live, partial]
    out["branches"] = sum(f.astype(np.int64) << b for b, f in enumerate(flags))
    return out


def finite_difference_accel(state, prev, dt, dtype=np.float64):
    """A13: a = (v - v_last)/dt, alpha likewise (hydrodynamics_behavior.py:196-202)."""
    state = np.asarray(state, dtype=dtype)
    prev = np.asarray(prev, dtype=dtype)
    return (state[:, 7:13] - prev) / float(dt)


def behavior_epilogue(position, comps, mass, dtype=np.float64):
    """Vectorised A14-A15 (hydrodynamics_behavior.py:212-226)."""
    p = np.asarray(position, dtype=dtype)
    arm_b = comps["center_of_buoyancy"] - p
    arm_p = comps["center_of_pressure"] - p
    net_f = (comps["buoyancy_force"] + comps["drag_force"] + comps["lift_force"]
             + comps["added_mass_force"])
    net_t = (np.cross(arm_b, comps["buoyancy_force"]) + np.cross(arm_p, comps["drag_force"])
             + np.cross(arm_p, comps["lift_force"]) + comps["drag_torque"]
             + comps["added_mass_torque"])
    f_mag = np.linalg.norm(net_f, axis=1)
    scale = np.minimum(1.0, np.asarray(mass, dtype=dtype) * MAX_ACCEL / (f_mag + CLAMP_EPS))
    return net_f * scale[:, None], net_t * scale[:, None], scale


def step_wrench(state, prev, params, rho, g, dt, semantics="numba", dtype=np.float64):
    """The fused entry point the HIP path implements: A13 + A1-A11 + A14 + A15, evaluated in `dtype`
    (see solve_components).

    Returns (net_force (N,3), net_torque (N,3), aux dict); aux['branches'] also has BRANCH_CLAMP set where the clamp
    acts (scale < 1)."""
    state = np.asarray(state, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    accel = finite_difference_accel(state, prev, dt, dtype)
    comps = solve_components(state, accel, params, rho, g, semantics, dtype)
    net_f, net_t, scale = behavior_epilogue(state[:, 0:3], comps, params[:, 10], dtype)
    comps["scale"] = scale
    net = comps["buoyancy_force"] + comps["drag_force"] + comps["lift_force"] + comps["added_mass_force"]
    comps["clamp_factor"] = params[:, 10] * MAX_ACCEL / (np.linalg.norm(net, axis=1) + CLAMP_EPS)    # before min(1, .)
    comps["branches"] = comps["branches"] | ((scale < 1.0).astype(np.int64) << BRANCH_CLAMP)
    return net_f, net_t, comps


def kinetic_energy(state, params, rotational=False):
    """sum 1/2 m |v|^2 (+ optional box-inertia rotational term).  New functionality
    named by BASELINE.json north_star; not present in the reference."""
    state = np.asarray(state, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64)
    m = params[:, 10]
    ke = 0.5 * m * np.einsum("na,na->n", state[:, 7:10], state[:, 7:10])
    if rotational:
        rot = _rot_batch(state[:, 3:7])
        d = params[:, 0:3]
        inertia = (m / 12.0)[:, None] * np.stack([d[:, 1] ** 2 + d[:, 2] ** 2,
                                                  d[:, 0] ** 2 + d[:, 2] ** 2,
                                                  d[:, 0] ** 2 + d[:, 1] ** 2], axis=1)
        w_b = np.einsum("nba,nb->na", rot, state[:, 10:13])
        ke = ke + 0.5 * np.einsum("na,na->n", inertia * w_b, w_b)
    return float(ke.sum()), ke


def wrench_error(net_f, net_t, ref_f, ref_t, params, rho, g):
    """Per-body error metric of SURVEY 8d:
    max(|dF| / max(|F_ref|, 1e-3 rho g V), |dT| / max(|T_ref|, 1e-3 rho g V L))."""
    params = np.asarray(params, dtype=np.float64)
    dims = params[:, 0:3]
    vol = dims.prod(axis=1)
    floor_f = 1e-3 * rho * g * vol
    floor_t = floor_f * dims.max(axis=1)
    e_f = np.linalg.norm(np.asarray(net_f, np.float64) - ref_f, axis=1) / np.maximum(np.linalg.norm(ref_f, axis=1), floor_f)
    e_t = np.linalg.norm(np.asarray(net_t, np.float64) - ref_t, axis=1) / np.maximum(np.linalg.norm(ref_t, axis=1), floor_t)
    return np.maximum(e_f, e_t)


# --------------------------------------------------------------------------
# per-component metric against a high-precision reference (tests/test_wrench_metric.py, tests/test_wrench_ulps_gpu.py)
# --------------------------------------------------------------------------
ULP = 2.0 ** -24              # unit roundoff of fp32: a correctly rounded y is within ULP * |y|
FLT_MIN = float(np.finfo(np.float32).tiny)
NORM_WEIGHT = 2.0 ** -20
# Non-clamped bodies: the kernels round each fp64 (1e-14-accurate) sum to fp32 ONCE, |y32 - y| <= ULP |y| <= ULP s_i.
# The norm part of s_i costs at most 2^-9 of a unit: the bound is 1 + 2^-8 by correct rounding, not a tuned number.
WRENCH_ULP_BOUND = 1.0 + 2.0 ** -8
# Clamp-active bodies: hydro_body.h assemble_wrench forms the clamp factor c = m 500 / (|F| + 1e-6) in fp32 and returns
# fl(c~ * fl(y)).  Relative errors, first order (1 ulp of an fp32 result <= 2^-23 of it = 2 ULP):
#   |F|^2 rounded to fp32                         ULP -> ULP/2 after the square root
#   v_sqrt_f32 (1 ulp)                            2 ULP        |F|~ : 2.5 ULP
#   + 1e-6f: the constant's own rounding (ULP, relative to its share of the sum) and the fp32 add (ULP)
#                                                  max(2.5, 1) + 1 = 3.5 ULP for the denominator
#   m * 500 in fp32                               ULP
#   v_rcp_f32 (1 ulp)                             2 ULP
#   the product                                   ULP          c~ : 3.5 + 1 + 2 + 1 = 7.5 ULP
#   fp32 rounding of y, then the product c~ * y   ULP + ULP
# -> |y_dev - c y| <= 9.5 ULP c |y| <= 9.5 ULP s_i (s_i carries the factor c), plus second-order terms (~1e-13) and the
# fp64 noise that 2^-8 covers.  fminf(1, .) is 1-Lipschitz, so a factor just above 1 on one side and just below on the
# other stays inside the same bound.  The host instantiation (libm's correctly rounded sqrt and division: ULP each)
# obeys 7.5 + 2^-8 by the same count.  Measured maxima over clamp-active bodies: host 4.07 (tests/test_wrench_metric.py),
# MI355X 4.44 (tests/test_wrench_ulps_gpu.py, every wrench entry); non-clamped: host 0.9972, MI355X 0.9972.
CLAMP_ULP_BOUND = 9.5 + 2.0 ** -8


def _abs_cross(a, f):
    """Component-wise |a x f| bound: (|a_y f_z| + |a_z f_y|, ...)."""
    a, f = np.abs(a), np.abs(f)
    return np.stack([a[:, 1] * f[:, 2] + a[:, 2] * f[:, 1], a[:, 2] * f[:, 0] + a[:, 0] * f[:, 2],
                     a[:, 0] * f[:, 1] + a[:, 1] * f[:, 0]], axis=1)


def wrench_scales(position, comps):
    """(s_force, s_torque), each (N,3): per component the sum of the magnitudes of the terms that form it, plus
    NORM_WEIGHT times the sum of the terms' norms, times the clamp scale.  Force terms: buoyancy, drag, lift, added
    mass.  Torque terms: the three lever-arm torques (as |a| x |F| component-wise, norm |a| |F|), drag torque, added-mass
    torque.  The norm part absorbs the ~1e-16 |F| residue of the rotation in components that are zero by symmetry."""
    p = np.asarray(position, dtype=comps["buoyancy_force"].dtype)
    nrm = lambda x: np.linalg.norm(x, axis=1)
    f_terms = [comps[k] for k in ("buoyancy_force", "drag_force", "lift_force", "added_mass_force")]
    s_f = sum(np.abs(x) for x in f_terms) + (NORM_WEIGHT * sum(nrm(x) for x in f_terms))[:, None]
    arms = [(comps["center_of_buoyancy"] - p, comps["buoyancy_force"]), (comps["center_of_pressure"] - p, comps["drag_force"]),
            (comps["center_of_pressure"] - p, comps["lift_force"])]
    s_t = (sum(_abs_cross(a, f) for a, f in arms) + np.abs(comps["drag_torque"]) + np.abs(comps["added_mass_torque"])
           + (NORM_WEIGHT * (sum(nrm(a) * nrm(f) for a, f in arms) + nrm(comps["drag_torque"])
                             + nrm(comps["added_mass_torque"])))[:, None])
    scale = comps["scale"][:, None]
    return s_f * scale, s_t * scale


def _component_ulps(got, ref, s):
    got = np.asarray(got, dtype=ref.dtype)
    d = np.abs(got - ref)
    # The device may flush fp32 denormals: a reference component below FLT_MIN is held to an absolute FLT_MIN.
    d = np.where(np.abs(ref) < FLT_MIN, np.maximum(d - FLT_MIN, 0.0), d)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 0.0, d / (ULP * s))              # s = 0 (no term at all): only an exact 0 passes
    return np.nan_to_num(e.astype(np.float64), nan=np.inf, posinf=np.inf).max(axis=1)


def wrench_error_ulps(got_f, got_t, ref, position):
    """Per-body worst force component and worst torque component of a device wrench, in units of ULP * s_i
    (wrench_scales).  `ref` = (net_force, net_torque, aux) from `step_wrench(..., dtype=np.longdouble)`, `position` the
    (N,3) positions it was evaluated at.  Returns {'force': (N,), 'torque': (N,), 'clamped': (N,) bool}.
    Bounds: WRENCH_ULP_BOUND where the clamp does not act, CLAMP_ULP_BOUND where it does.  'clamped' is scale < 1, and
    also a factor below 1 + 2^-20: the kernels' fp32 factor (7.5 ULP, see CLAMP_ULP_BOUND) can fall below 1 there."""
    ref_f, ref_t, comps = ref
    s_f, s_t = wrench_scales(position, comps)
    return {"force": _component_ulps(got_f, ref_f, s_f), "torque": _component_ulps(got_t, ref_t, s_t),
            "clamped": np.asarray(comps["clamp_factor"] < 1.0 + 2.0 ** -20)}


def branch_flips(aux_a, aux_b):
    """Bodies on which two evaluations (fp64 and longdouble) took a different decision (BRANCH_NAMES), and the names of
    the decisions that differ, as {body index: [names]}."""
    diff = np.asarray(aux_a["branches"]) ^ np.asarray(aux_b["branches"])
    return {int(i): [nm for b, nm in enumerate(BRANCH_NAMES) if (int(diff[i]) >> b) & 1] for i in np.nonzero(diff)[0]}
