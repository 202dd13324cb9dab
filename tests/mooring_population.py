"""The mooring lines of the designed population (designed_populations.bed_pop with a line per body), the fixture that carries them,
and config 1's buoy on its line: shared by tests/test_mooring.py, test_extremes.py, test_symmetry.py and their GPU counterparts.
"""
import numpy as np
import pytest

import mooring_reference as mr
import populations
from designed_populations import bed_population
from silver2_isaacsim_amd import scenes

NONE_TILE, ALL_TILE = 2, 1                                         # (the bed's population: nobody touches in tile 1, everybody in tile 2)
TIES = np.arange(8)                                                # l within 2 fp32 ulps of L0: 0 .. 3 with c = 0, 4 .. 7 with c > 0
TIE_ULPS = (-2, -1, 1, 2, -2, -1, 1, 2)                            # L0 - l, in ulps of l: negative = taut
CLAMPED = 64 + np.arange(8)                                        # taut, the fairlead closing in so fast that T clamps to 0


def line_population(st, pr, seed=2027):
    """A line per body of the 321-body population of tests/test_seabed_gpu.py, built from each body's own state: the anchor is
    the fairlead's world position + a drawn direction x L (L = 2 .. 30 m), L0 = L (1 -+ margin), margin 1e-3 .. 0.1; k and c per
    unit mass up to 14.4 / s^2 and 1.2 / s (the defaults at 60 Hz).  Returns the (321, 9) float32 record:
      bodies 0 .. 7          : l within 2 fp32 ulps of L0 (TIE_ULPS), the fairlead running away from the anchor; 0 .. 3 with c = 0
      the rest of tile 0     : slack, but four in every sixteen taut
      tile 1 (64 .. 127)     : all taut; 64 .. 71 with a fairlead that closes in fast enough for T to clamp to 0, the others pulling
                               (no body of this tile touches the bed of tests/test_seabed_gpu.py: lines alone)
      tile 2 (128 .. 191)    : no lines (the wave skips the evaluation; every body of this tile touches the bed: the bed alone)
      192 .. 199             : slack
      200 .. 319             : in turn taut and pulling, slack, no line
      320                    : the one live lane of the last wave, taut and pulling."""
    n = len(st)
    assert n == 321
    rng = np.random.default_rng(seed)
    st64 = np.asarray(st, np.float64)
    i = np.arange(n)
    tile = i // 64
    TAUT, SLACK, NONE = 0, 1, 2
    kind = np.where(tile == NONE_TILE, NONE, np.where(tile == ALL_TILE, TAUT, np.where(tile == 0, np.where(i % 4 == 1, TAUT, SLACK),
                                                                                      np.where(i < 200, SLACK, (i - 200) % 3))))
    kind[320] = TAUT
    kind[TIES] = TAUT
    rec = np.zeros((n, 9))
    rec[:, 3:6] = rng.uniform(-0.5, 0.5, (n, 3)) * pr[:, 0:3]                      # fairleads within the box
    rec0 = rec.copy()
    r, _, _, _, u, _ = mr.geometry(rec0, st64)                                     # (the arm and the fairlead's velocity do not depend on the anchor)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    speed = np.linalg.norm(u, axis=1)
    away = np.where(speed[:, None] > 0, -u / np.maximum(speed, 1e-30)[:, None], d)
    d[TIES] = away[TIES]                                                          # e along -u: the fairlead runs away (un < 0), so a taut tie pulls
    d[CLAMPED] = -away[CLAMPED]                                                   # e along +u: it closes in at its full speed
    assert (speed[TIES] > 1e-4).all() and (speed[CLAMPED] > 1e-3).all()
    L = rng.uniform(2.0, 30.0, n)
    margin = 10.0 ** rng.uniform(-3.0, -1.0, n)
    margin[CLAMPED] = 1e-3
    rec[:, 0:3] = st64[:, 0:3] + r + d * L[:, None]
    rec[:, 6] = np.where(kind == SLACK, L * (1.0 + margin), L * (1.0 - margin))
    m = pr[:, 10].astype(np.float64)
    rec[:, 7] = np.where(kind == NONE, 0.0, m * rng.uniform(0.5, 14.4, n))
    rec[:, 8] = np.where(kind == NONE, 0.0, m * rng.uniform(0.0, 1.2, n) * (i % 5 != 0))          # one line in five without a damper
    rec = rec.astype(np.float32).astype(np.float64)
    # taut and meant to pull: keep the damper below half the spring's force
    _, _, _, x, _, un = mr.geometry(rec, st64)
    pull = (kind == TAUT) & ~np.isin(i, CLAMPED) & ~np.isin(i, TIES)
    too_much = pull & (rec[:, 8] * un > 0.5 * rec[:, 7] * x)
    rec[too_much, 8] = 0.5 * rec[too_much, 7] * x[too_much] / un[too_much]
    rec[CLAMPED, 8] = 4.0 * rec[CLAMPED, 7] * x[CLAMPED] / un[CLAMPED]             # c un = 4 k x
    rec[TIES[:4], 8] = 0.0
    rec[TIES[4:], 8] = np.maximum(rec[TIES[4:], 8], 0.3 * m[TIES[4:]])
    rec = rec.astype(np.float32)
    # the ties: L0 is the kernel's own l moved by whole fp32 steps
    free = rec.copy()
    free[:, 6] = 0.0
    l32 = mr._fp32_terms(free, st)[3]                                             # x with L0 = 0: l itself
    for b, k in zip(TIES, TIE_ULPS):
        v = l32[b]
        for _ in range(abs(k)):
            v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
        rec[b, 6] = v
    return rec


def designed_population():
    """(state, prev, params f32, record) of the 321 bodies, built without a device."""
    st, pv, pr = populations.integrator_population(n=4097, seed=31)
    st, pv, pr = bed_population(st, pv, pr)
    return st, pv, pr, line_population(st, pr)


def population_report(rec, st):
    """What the population is made of, by the fp64 reference: (taut and pulling, slack, no line, taut and clamped)."""
    has, on, T = mr.has_line(rec), mr.taut(rec, st), mr.tension(rec, st)
    return on & (T > 0), has & ~on, ~has, on & ~(T > 0)


DEPTH = 20.0                                                       # the anchor, below the buoy's equilibrium position (m)


def buoy():
    """Config 1's buoy at rest at its draught: (state, prev, params, scene, dt, z_eq, mass)."""
    sc = scenes.scene_c1()
    pr = sc.params[:1].astype(np.float32)
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (sc.rho * float(pr[0, 0] * pr[0, 1]))
    st = np.zeros((1, 13), np.float32)
    st[0, 2], st[0, 6] = z_eq, 1.0
    return st, np.zeros((1, 6), np.float32), pr, sc, float(np.float32(1.0 / 60.0)), z_eq, mass


OFF_TIES = ~np.isin(np.arange(321), TIES)


@pytest.fixture(scope="module")
def moored_pop(bed_pop):
    st, pv, params, applied, ctl = bed_pop
    return st, pv, params, applied, ctl, line_population(st, params["f32"])


def _buoys():
    """64 copies of config 1's buoy at rest at their draught, 50 m apart, copy i turned by i / 64 of a revolution about z."""
    st, pv, pr, sc, dt, z_eq, mass = buoy()
    i = np.arange(64)
    st, pv, pr = np.tile(st, (64, 1)), np.tile(pv, (64, 1)), np.tile(pr, (64, 1))
    st[:, 0], st[:, 1] = 50.0 * (i % 8), 50.0 * (i // 8)
    yaw = 2.0 * np.pi * i / 64.0
    st[:, 5], st[:, 6] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
    anchors = np.stack([st[:, 0], st[:, 1], np.full(64, z_eq - DEPTH)], axis=1).astype(np.float64)
    return scenes.Scene("buoys", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g), anchors, z_eq, mass
