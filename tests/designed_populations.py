"""The designed populations, scenes and pytest fixtures the feature tests share, CPU and GPU alike.  The populations form a chain,
each the previous one with one more record: the integrator population with an applied wrench and a pose-hold record (`hold_pop`)
-> moved onto the displaced surface (`sea_pop`) or onto the bed (`bed_pop`) -> with mooring lines (mooring_population.moored_pop)
-> with tethers (tether_population).  A fixture is defined once, here or in those two modules; a test module imports it under the
name it requests it by, together with the fixtures it is built from.
"""
import math

import numpy as np
import pytest

import populations
import pose_hold_reference as phr
import resident_harness
import seabed_reference as br
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed
from silver2_isaacsim_amd.testing import build_main_scene

RHO, G, DT = populations.RHO, populations.G, populations.DT


# ---- the sea ---------------------------------------------------------------------------------------------------------------------------
def _test_sea():
    sea = SeaState((0.5, -0.2, 0.05))
    for lam, head, a, ph in ((100.0, 20.0, 0.2, 0.3), (25.0, -70.0, 0.1, 1.1), (8.0, 160.0, 0.05, -2.0)):
        kappa = 2.0 * math.pi / lam
        sea.add_wave(a, kappa * math.cos(math.radians(head)), kappa * math.sin(math.radians(head)), math.sqrt(9.81 * kappa), ph)
    return sea


def drift_scene():
    """A neutrally buoyant 0.5 m cube at z = -10 m, README coefficients, at rest; the current it is released into."""
    st = np.zeros((1, 13), np.float32)
    st[0, 2], st[0, 6] = -10.0, 1.0
    pr = np.concatenate([[0.5, 0.5, 0.5], scenes._DEFAULT_COEFFS, [scenes.RHO * 0.125]])[None, :].astype(np.float32)
    return st, np.zeros((1, 6), np.float32), pr, SeaState((0.5, 0.2, 0.0))


def wave_scene():
    """Config 1's buoy (unit cube, 500 kg) and the wave it rides: a = 0.2 m, T = 8 s, along +x; its equilibrium z."""
    sc = scenes.scene_c1()
    return sc, SeaState.regular(0.4, 8.0, 0.0), 0.5 - 500.0 / scenes.RHO


SEA = _test_sea()              # U = (0.5, -0.2, 0.05); components of 100, 25 and 8 m wavelength at different headings, a = 0.2 .. 0.05 m


@pytest.fixture(scope="module")
def hold_pop():
    """The designed population of the applied-wrench tests with its applied wrench, and a control record per body:
    targets up to 2 m and up to 2.4 rad away (half of the target quaternions written with the opposite sign, so that both
    sides of the law's sign flip occur; every |q_e.w| >= 0.1), gains per unit mass / inertia of 5 .. 50 s^-2 and 1 .. 10 s^-1
    (one axis in eight without a linear gain), and limits: body 6k saturates f_max, body 6k + 3 saturates t_max (at 0.1 .. 0.9
    of the unclamped norm), the others are unlimited or stay below twice their unclamped norm."""
    st, pv, pr = populations.integrator_population(n=max(resident_harness.SIZES), seed=31)
    n = len(st)
    params = {"f32": pr, "f16": pr.copy()}
    params["f16"][:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(77)
    top = 50.0 * pr[:, 10:11].astype(np.float64)
    applied = np.concatenate([rng.uniform(-1, 1, (n, 3)) * top,
                              rng.uniform(-1, 1, (n, 3)) * top * pr[:, 0:3].max(axis=1, keepdims=True)], axis=1).astype(np.float32)
    rng = np.random.default_rng(78)
    mass = pr[:, 10:11].astype(np.float64)
    inertia = io.box_inertia(pr.astype(np.float64)).mean(axis=1)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.0, 2.4, (n, 1))
    dq = np.concatenate([np.sin(half) * axis, np.cos(half)], axis=1)
    q = st[:, 3:7].astype(np.float64)
    target_q = np.concatenate([dq[:, 3:4] * q[:, 0:3] + q[:, 3:4] * dq[:, 0:3] + np.cross(dq[:, 0:3], q[:, 0:3]),
                               dq[:, 3:4] * q[:, 3:4] - np.sum(dq[:, 0:3] * q[:, 0:3], axis=1, keepdims=True)], axis=1)
    target_q *= np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    kp_lin = mass * rng.uniform(5.0, 50.0, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.125)
    ctl = phr.record(n, st[:, 0:3].astype(np.float64) + rng.uniform(-2.0, 2.0, (n, 3)), target_q, kp_lin, mass * rng.uniform(1.0, 10.0, (n, 3)),
                     inertia * rng.uniform(5.0, 50.0, n), inertia * rng.uniform(1.0, 10.0, n))
    force, torque = phr.unclamped(st, ctl)
    which, frac = np.arange(n) % 6, rng.uniform(0.1, 0.9, n)
    ctl[:, phr.F_MAX] = np.where(which == 0, frac * np.linalg.norm(force, axis=1), np.where(which == 1, 2.0 * np.linalg.norm(force, axis=1), np.inf))
    ctl[:, phr.T_MAX] = np.where(which == 3, frac * np.linalg.norm(torque, axis=1), np.where(which == 4, 2.0 * np.linalg.norm(torque, axis=1), np.inf))
    cache = {}

    def comps(coeff):
        if coeff not in cache:
            cache[coeff] = ho.step_wrench(st, pv, params[coeff], RHO, G, DT)[2]
        return cache[coeff]
    return st, pv, params, applied, ctl, comps


@pytest.fixture(scope="module")
def sea_pop(hold_pop):
    """The designed population of the applied-wrench and pose-hold tests, every body moved up or down by the surface
    elevation above it at t = 0, so that the partial ones straddle the DISPLACED surface."""
    st, pv, params, applied, ctl, _ = hold_pop
    st = st.copy()
    st[:, 2] = (st[:, 2].astype(np.float64) + SEA.elevation(st[:, 0], st[:, 1], 0.0)).astype(np.float32)
    return st, pv, params, applied, ctl


SIZES = (200, 321)
STEPS = (1, 7)
Z_BED = -3.0
BED = Seabed.for_step(Z_BED, DT)
FAR = Seabed.for_step(-1e6, DT)
NEAR = np.arange(8)                                               # the bodies whose lowest corner stands within an ulp of the plane
NONE_TILE, ALL_TILE = 1, 2


def _lowest_fp32(st, pr):
    """p_z - ((|A_z| + |B_z|) + |C_z|) as the kernel forms it, in NumPy float32 (no fused operation in it)."""
    x, y, z, w = (st[:, 3 + i] for i in range(4))
    r20, r21, r22 = x * (z + z) - w * (y + y), y * (z + z) + w * (x + x), np.float32(1) - (x * (x + x) + y * (y + y))
    half = np.float32(0.5)
    reach = (np.abs(half * (r20 * pr[:, 0])) + np.abs(half * (r21 * pr[:, 1]))) + np.abs(half * (r22 * pr[:, 2]))
    return st[:, 2] - reach, reach


def bed_population(st, pv, pr):
    """The first 321 bodies of the designed population (every attitude, 5 % of the quaternions non-unit, |v| up to 5 m/s,
    |omega| up to 10 rad/s, slabs up to 1:10) moved in z only, so that against the plane z = Z_BED
      bodies 0 .. 7          : the lowest corner stands at Z_BED + (-1, 0, 1, -1, 0, 1, -1, 0) fp32 ulps of Z_BED, in the kernel's
                               own arithmetic - the decision delta > 0 at its tie
      the rest of tile 0     : alternately 1 .. 3 and 4 .. 8 corners below the plane
      tile 1 (64 .. 127)     : nobody reaches the plane (the wave skips the contact)
      tile 2 (128 .. 191)    : everybody touches, alternately 1 .. 3 and 4 .. 8 corners
      192 .. 319             : in turn none, 1 .. 3, 4 .. 8
      320                    : the one live lane of the last wave, 4 .. 8 corners."""
    n = 321
    st, pv, pr = st[:n].copy(), pv[:n].copy(), pr[:n].copy()
    rng = np.random.default_rng(2026)
    st[:, 2] = 0.0
    h = np.sort(br.corners(st, pr)[:, :, 2], axis=1)             # corner heights above the centre, ascending
    i = np.arange(n)
    tile = i // 64
    kind = np.where(tile == NONE_TILE, 0, np.where((tile == 0) | (tile == ALL_TILE), 1 + i % 2, i % 3))      # 0 none, 1 few, 2 many
    kind[320] = 2
    f = rng.uniform(0.15, 0.85, n)
    plane_above_centre = np.where(kind == 0, h[:, 0] - rng.uniform(0.05, 0.4, n),
                                  np.where(kind == 1, h[:, 0] + f * (h[:, 3] - h[:, 0]), h[:, 3] + f * (h[:, 7] - h[:, 3])))
    st[:, 2] = (Z_BED - plane_above_centre).astype(np.float32)
    # the eight at the tie: move p_z by single fp32 steps until the kernel's lowest corner is the wanted neighbour of Z_BED
    zb = np.float32(Z_BED)
    for b, k in zip(NEAR, (-1, 0, 1, -1, 0, 1, -1, 0)):
        want = zb
        for _ in range(abs(k)):
            want = np.nextafter(want, np.float32(np.inf if k > 0 else -np.inf))
        one = st[b:b + 1]
        one[0, 2] = want + _lowest_fp32(one, pr[b:b + 1])[1][0]
        for _ in range(64):
            low = _lowest_fp32(one, pr[b:b + 1])[0][0]
            if low == want:
                break
            one[0, 2] = np.nextafter(one[0, 2], np.float32(np.inf if low < want else -np.inf))
        assert _lowest_fp32(one, pr[b:b + 1])[0][0] == want, b
    return st, pv, pr


@pytest.fixture(scope="module")
def bed_pop(hold_pop):
    st, pv, params, applied, ctl, _ = hold_pop
    st, pv, pr = bed_population(st, pv, params["f32"])
    n = len(st)
    p16 = params["f16"][:n].copy()
    return st, pv, {"f32": pr, "f16": p16}, applied[:n].copy(), ctl[:n].copy()


Z_B = -5.0
BOXES = (((0.5, 0.5, 0.5), 2.0), ((1.0, 1.0, 1.0), 1.05), ((0.8, 0.3, 0.2), 1.3), ((0.3, 0.2, 0.1), 7.8))     # dimensions (m), rho_body / rho
REST_V, REST_W, REST_Z, PENETRATION = 1e-4, 1e-4, 1e-4, 0.15


def _quat(axis, angle):
    q = np.zeros(4)
    q[axis], q[3] = np.sin(angle / 2), np.cos(angle / 2)
    return q


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


ATTITUDES = {"flat": _quat(0, 0.0), "tilted": _qmul(_quat(1, 0.35), _quat(0, 0.5)), "edge": _quat(0, np.pi / 4)}


def settling_boxes():
    """The twelve boxes (four boxes x flat / tilted by 0.5 rad about x then 0.35 rad about y / on an edge), README coefficients,
    released with their centre 1 m above the bed and v_x = 0.3 m/s: (state, prev, params, rho_body / rho per box)."""
    st, pr, ratios = [], [], []
    for dims, ratio in BOXES:
        for q in ATTITUDES.values():
            s = np.zeros(13)
            s[2], s[3:7], s[7] = Z_B + 1.0, q, 0.3
            st.append(s)
            pr.append(np.concatenate([dims, scenes._DEFAULT_COEFFS, [ratio * scenes.RHO * np.prod(dims)]]))
            ratios.append(ratio)
    return np.array(st, np.float32), np.zeros((len(st), 6), np.float32), np.array(pr, np.float32), np.array(ratios)


def rest_report(bed, state, params, ratios, g=scenes.G):
    """Per box: corners in contact, |v|, |omega|, and how far the lowest corner is from z_b - g (1 - rho / rho_body) / (4 kappa)."""
    delta = br.penetration(bed, state, params)
    st = np.asarray(state, np.float64)
    return ((delta > 0).sum(axis=1), np.linalg.norm(st[:, 7:10], axis=1), np.linalg.norm(st[:, 10:13], axis=1),
            np.abs(delta.max(axis=1) - g * (1.0 - 1.0 / ratios) / (4.0 * bed.stiffness)))


def contributing_corners(st, pr, bed=BED):
    """(n,) the most corners seabed_reference counts on a body over `bed`: decided in fp64 and as the kernel decides, whichever is more."""
    return np.maximum(br.corner_count(bed, st, pr), br.corner_count(bed, st, pr, br.touching_fp32(bed, st, pr)))


def tilted_boxes(st, pv, pr, seed=2028):
    """The bed population with four bodies in five lowered or raised, in z only, so that exactly ONE corner is below the plane
    (between its lowest and its second-lowest corner) - but for bodies 0 .. 7 (the ties) and tile 1, which nobody touches in:
    the bed population itself draws 1 .. 3 corners together and leaves the single-corner bodies, on which the device is exact,
    to chance.  A population of this module; the feature tests' population is not touched."""
    st = st.copy()
    rng = np.random.default_rng(seed)
    flat = st.copy()
    flat[:, 2] = 0.0
    h = np.sort(br.corners(flat, pr)[:, :, 2], axis=1)
    i = np.arange(len(st))
    one = (i % 5 != 1) & (i >= 8) & (i // 64 != 1) & (h[:, 1] - h[:, 0] > 1e-3)
    f = rng.uniform(0.2, 0.8, len(st))
    z = float(BED.z) - (h[:, 0] + f * (h[:, 1] - h[:, 0]))
    st[one, 2] = z[one].astype(np.float32)
    return st, pv.copy(), pr.copy()


def build_scene(batched, config_path=None, seed=0):
    """The 20 prims of silver2_isaac_sim.usd that carry the behavior."""
    return build_main_scene(batched, config_path, seed)
