"""The trajectory recorder on the device: every recorded row is, bit for bit, the state single-step eager stepping leaves
in memory at that step (and the wrench of the step that produced it); recording changes nobody's bits; the log is touched
nowhere else; refusals happen before anything is launched.  No tolerance anywhere except the one config 1 has always had
against its fp64 golden trajectory."""
import csv
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd._native import HydroError
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from silver2_isaacsim_amd.telemetry import CSV_HEADER, write_velocity_log

pytestmark = pytest.mark.gpu
FILL = -777.25                                                   # what the tests put into a log before a run


def _sim(sc, semantics="numba", **kw):
    sim = ClosedLoopSim(sc, **kw)
    if semantics != "numba":
        sim.engine.set_semantics(semantics)
    return sim


def eager_reference(sc, steps, semantics="numba", **kw):
    """(steps, n, 13) states after each step of ClosedLoopSim.run_eager(1), and (steps, n, 6) wrenches of each step from
    hydro_step_fused_tiled(..., wrench=w) on a second sim stepped by hand (whose states must be the first one's)."""
    a, b = _sim(sc, semantics, **kw), _sim(sc, semantics, **kw)
    w = b.engine.alloc_tiled(6, sc.n)
    states, wrenches = [], []
    for _ in range(steps):
        a.run_eager(1)
        states.append(a.state())
        with torch.cuda.stream(b.stream):
            b.engine.step_fused_tiled(b.cur, b.old, sc.n, sc.dt, wrench=w, implicit_drag=b.implicit_drag)
        b.cur, b.old = b.old, b.cur
        b.steps_done += 1
        assert np.array_equal(b.state(), states[-1], equal_nan=True)
        wrenches.append(scenes.from_tiled(w.cpu().numpy(), sc.n))
    a.close(); b.close()
    return np.stack(states), np.stack(wrenches)


def final_bits(sim):
    """Everything a run leaves behind: the current state and the other buffer (its velocity fields are `prev`)."""
    sim.synchronize()
    return scenes.from_tiled(sim.cur.cpu().numpy(), sim.n), scenes.from_tiled(sim.old.cpu().numpy(), sim.n)[:, 7:13]


def watch_list(n):
    """All 64 bodies of one tile, single bodies in the first and in the last tile - the last body of all among them -
    in an order that is not the library's."""
    tiles = (n + 63) // 64
    mid = (tiles // 2) * 64
    return [n - 1, 5] + list(range(mid, mid + 64))[::-1] + [0, (tiles - 1) * 64]


CASES = {
    # name: (scene, steps, sim kwargs, semantics)
    "c2 n=1000 f32 explicit": (lambda: scenes.scene_c2(n=1000), 200, {}, "numba"),
    "c5 n=3000 f16 explicit": (lambda: scenes.scene_c5(n=3000), 4, {"coeff_dtype": "f16"}, "numba"),     # light bodies: 4 steps
    "c3 sample implicit drag": (lambda: scenes.scene_c3(envs=64), 200, {"implicit_drag": True}, "numba"),
    "c2 n=1000 warp semantics": (lambda: scenes.scene_c2(n=1000), 200, {}, "warp"),
}
_REFERENCE = {}


def reference(name):
    if name not in _REFERENCE:
        make, steps, kw, sem = CASES[name]
        _REFERENCE[name] = eager_reference(make(), steps, sem, **kw)
    return _REFERENCE[name]


def check_recorded(name, every, chunk, runner="resident", wrench=True, ke_every=0):
    make, steps, kw, sem = CASES[name]
    sc = make()
    ref_states, ref_wrenches = reference(name)
    bodies = watch_list(sc.n)
    assert sc.n % 64 != 0 or name.startswith("c3")               # the last body sits in a partial tile (c2, c5)
    kw = dict(kw, ke_every=ke_every) if ke_every else kw
    sim, plain = _sim(sc, sem, **kw), _sim(sc, sem, **kw)
    rows = steps // every + 3                                     # three rows more than the run needs: they must stay untouched
    rec = sim.record(bodies, every=every, rows=rows, wrench=wrench)
    rec.log.fill_(FILL)
    if runner == "resident":
        sim.run_resident(steps, chunk=chunk)
    else:
        sim.run_eager(steps)
    plain.run_resident(steps, chunk=chunk)
    # steps(): exactly the multiples of `every`
    want_steps = list(range(every, steps + 1, every))
    assert list(rec.steps()) == want_steps and rec.rows_written == len(want_steps)
    got = rec.states()
    assert got.shape == (len(want_steps), len(bodies), 13)
    for r, k in enumerate(want_steps):
        assert np.array_equal(got[r], ref_states[k - 1][bodies], equal_nan=True), (name, every, chunk, "state after step", k)
    if wrench:
        gw = rec.wrenches()
        for r, k in enumerate(want_steps):
            assert np.array_equal(gw[r], ref_wrenches[k - 1][bodies], equal_nan=True), (name, every, chunk, "wrench of step", k)
    # nothing else in the log moved
    assert (rec.log[rec.rows_written:] == FILL).all()
    # recording changed nobody's bits: final state, prev, kinetic-energy samples of a run without a recorder
    (s1, p1), (s0, p0) = final_bits(sim), final_bits(plain)
    assert np.array_equal(s1, s0, equal_nan=True) and np.array_equal(p1, p0, equal_nan=True)
    assert np.array_equal(s1, ref_states[-1], equal_nan=True)
    if ke_every:
        sim.monitor.collect(block=True); plain.monitor.collect(block=True)
        assert len(plain.monitor.samples) == steps // ke_every > 0
        assert sim.monitor.samples == plain.monitor.samples
    sim.close(); plain.close()
    return rec


@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("chunk", [48, 64])
def test_recorded_rows_are_the_eager_states_c2(every, chunk, native_built):
    """200 steps in launches of 48 / 64 (+ a remainder of 8): samples fall on first, middle and last steps of launches."""
    check_recorded("c2 n=1000 f32 explicit", every, chunk)


def test_launches_without_a_sample(native_built):
    """every = 100 with chunks of 48: launches 1, 2 and 4 hold no sample at all (phase > steps), launch 3 and 5 one each."""
    rec = check_recorded("c2 n=1000 f32 explicit", 100, 48)
    assert rec.rows_written == 2


@pytest.mark.parametrize("name,every,chunk", [("c5 n=3000 f16 explicit", 1, 3), ("c5 n=3000 f16 explicit", 2, 4),
                                              ("c3 sample implicit drag", 5, 64), ("c3 sample implicit drag", 1, 48),
                                              ("c2 n=1000 warp semantics", 5, 48)])
def test_recorded_rows_are_the_eager_states_other_variants(name, every, chunk, native_built):
    check_recorded(name, every, chunk)


def test_state_only_log_and_kinetic_energy_samples(native_built):
    """13-field log (no wrench) next to a kinetic-energy monitor sampling every 64 steps: the KE instantiation of the
    recording kernel leaves the monitor's samples of the plain one."""
    check_recorded("c2 n=1000 f32 explicit", 5, 64, wrench=False, ke_every=64)
    check_recorded("c3 sample implicit drag", 1, 64, wrench=True, ke_every=64)


@pytest.mark.parametrize("every", [1, 5])
def test_eager_stepping_records_the_same_log(every, native_built):
    a = check_recorded("c2 n=1000 f32 explicit", every, 64, runner="eager")
    b = check_recorded("c2 n=1000 f32 explicit", every, 64, runner="resident")
    assert torch.equal(a.log, b.log)


def test_recorder_attached_in_mid_run_and_rewound(native_built):
    ref_states, _ = reference("c2 n=1000 f32 explicit")
    sim = ClosedLoopSim(scenes.scene_c2(n=1000))
    sim.run_resident(12, chunk=64)
    rec = sim.record([999, 64], every=5, rows=8)
    sim.run_resident(30, chunk=7)                                # steps 13 .. 42: samples after 15, 20, ... 40
    assert list(rec.steps()) == [15, 20, 25, 30, 35, 40]
    assert np.array_equal(rec.states(), ref_states[[14, 19, 24, 29, 34, 39]][:, [999, 64]])
    rec.rewind()
    sim.run_resident(8, chunk=64)                                # steps 43 .. 50
    assert list(rec.steps()) == [45, 50] and np.array_equal(rec.states(), ref_states[[44, 49]][:, [999, 64]])
    sim.stop_recording()
    assert sim.engine.watch_count == 0
    sim.run_resident(10, chunk=64)
    assert np.array_equal(sim.state(), ref_states[59])
    sim.close()


def test_wide_log_keeps_the_columns_nobody_owns(native_built):
    """log_stride > count through the engine entry: columns >= count and rows beyond those written keep the fill value."""
    sc = scenes.scene_c2(n=1000)
    ref_states, ref_wrenches = reference("c2 n=1000 f32 explicit")
    sim = ClosedLoopSim(sc)
    e = sim.engine
    bodies = [3, 64, 65, 999]
    assert e.set_watch(bodies) == 4 and e.watch_count == 4
    log = torch.full((12, 19, 7), FILL, dtype=torch.float32, device=e.device)
    with torch.cuda.stream(sim.stream):
        rows = e.step_fused_tiled_multi_rec(sim.cur, sim.old, sc.n, sc.dt, 20, log, every=3, phase=2, row0=4)
    sim.synchronize()
    assert rows == 7                                             # after local steps 2, 5, 8, 11, 14, 17, 20 -> rows 4 .. 10
    host = log.cpu().numpy()
    for i, k in enumerate(range(2, 21, 3)):
        assert np.array_equal(host[4 + i, :13, :4].T, ref_states[k - 1][bodies])
        assert np.array_equal(host[4 + i, 13:, :4].T, ref_wrenches[k - 1][bodies])
    assert (host[:4] == FILL).all() and (host[11:] == FILL).all() and (host[:, :, 4:] == FILL).all()
    sim.close()


# ---- config 1, end to end ----------------------------------------------------------------------------------------------------
def test_config1_buoy_recorded_at_every_step(native_built, tmp_path):
    """The buoy of config 1 recorded at every one of 10 000 steps inside ten resident launches of 1 000.  Row k - 1 is the
    state after step k, as is z[k - 1] of tests/golden/c1_trajectory.npz (the reference's functions, fp64).
    The rows 99::100 are the sample points of test_config1_single_buoy_on_the_gpu and, by the bit equalities above, the
    same numbers: 6.6e-8 m against its bound of 1e-6 m.  The rows in between had never been seen before this recorder:
    measured on an MI355X, the maximum over ALL 10 000 rows is 7.9e-8 m (row 8464; v_z within 3.3e-7 m/s) - the same
    order of magnitude of margin, so every row is held to the same 1e-6 m."""
    fx = load_golden("c1_trajectory")
    sim, plain = ClosedLoopSim(scenes.scene_c1()), ClosedLoopSim(scenes.scene_c1())
    rec = sim.record([0], every=1, rows=10000)
    sim.run_resident(10000, chunk=1000)
    plain.run_resident(10000, chunk=1000)
    st = rec.states()
    assert st.shape == (10000, 1, 13) and list(rec.steps()) == list(range(1, 10001))
    z = st[:, 0, 2].astype(np.float64)
    sampled, everywhere = np.abs(z[99::100] - fx["z"][99::100]).max(), np.abs(z - fx["z"]).max()
    print(f"[config 1, recorded] max |z - z_ref|: {sampled:.3e} m at rows 99::100, {everywhere:.3e} m over all 10 000 rows "
          f"(row {int(np.abs(z - fx['z']).argmax())}); max |v_z - v_z_ref| {np.abs(st[:, 0, 9] - fx['vz']).max():.3e} m/s")
    assert sampled < 1e-6, sampled
    assert everywhere < 1e-6, everywhere
    assert np.array_equal(st[-1, 0], sim.state()[0]) and np.array_equal(sim.state(), plain.state())
    # the reference's artefact from the device log: parses back to the recorded floats exactly
    path = write_velocity_log(str(tmp_path), rec, 0, dt=sim.dt)
    rows = list(csv.reader(open(path)))
    assert rows[0] == CSV_HEADER and len(rows) == 10001
    back = np.array([[float(x) for x in r[1:]] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(back, st[:, 0, [2, 9, 12, 0, 7, 10, 1, 8, 11]])
    sim.close(); plain.close()


# ---- refusals: status codes and ValueErrors, nothing launched, nothing written ---------------------------------------------------
def _raw_rec(sim, log, n=None, steps=4, fields=None, stride=None, rows=None, every=1, phase=1, row0=0):
    """hydro_step_fused_tiled_multi_rec with nothing between the test and the C entry."""
    e = sim.engine
    st, vel = 13 * 64, 7 * 64 * 4
    written = ctypes.c_int64(-7)
    rc = e._lib.hydro_step_fused_tiled_multi_rec(
        e._h, sim.n if n is None else n, sim.cur.data_ptr(), st, sim.old.data_ptr() + vel, st, float(sim.dt), steps,
        sim.old.data_ptr(), st, sim.cur.data_ptr() + vel, st, 0, 1, None,
        log.data_ptr(), log.shape[2] if stride is None else stride, log.shape[0] if rows is None else rows,
        log.shape[1] if fields is None else fields, every, phase, row0, ctypes.byref(written), e._stream(sim.stream))
    return rc, written.value


def test_refusals_launch_nothing(native_built):
    sc = scenes.scene_c2(n=1000)
    sim = ClosedLoopSim(sc)
    e = sim.engine
    before = (sim.cur.clone(), sim.old.clone())
    log = torch.full((8, 19, 6), FILL, dtype=torch.float32, device=e.device)
    E_ARG, E_STATE = -1, -5
    assert _raw_rec(sim, log) == (E_STATE, -7)                   # no watch list
    with pytest.raises(HydroError) as err:
        e.step_fused_tiled_multi_rec(sim.cur, sim.old, sc.n, sc.dt, 4, log, 1, 1, 0)
    assert err.value.status == E_STATE
    # bad lists: refused, the previous list stays in force
    assert e.set_watch([2, 500, 999]) == 3
    for bad in ([5, 4], [4, 4], [0, 1000], [-1, 3], list(range(nat.WATCH_MAX + 1))):
        with pytest.raises(HydroError) as err:
            e.set_watch(bad)
        assert err.value.status == E_ARG and e.watch_count == 3
    # bad launches
    assert _raw_rec(sim, log, n=999)[0] == E_ARG                 # a watched body (999) >= n
    assert _raw_rec(sim, log, fields=14)[0] == E_ARG
    assert _raw_rec(sim, log, stride=2)[0] == E_ARG              # log_stride < count
    assert _raw_rec(sim, log, every=0)[0] == E_ARG
    assert _raw_rec(sim, log, every=3, phase=4)[0] == E_ARG and _raw_rec(sim, log, every=3, phase=0)[0] == E_ARG
    assert _raw_rec(sim, log, steps=9)[0] == E_ARG               # rows 0 .. 8 of 8
    assert _raw_rec(sim, log, steps=4, row0=5)[0] == E_ARG       # rows 5 .. 8 of 8
    assert _raw_rec(sim, log, steps=0)[0] == E_ARG
    sim.synchronize()
    assert (log == FILL).all() and torch.equal(sim.cur, before[0]) and torch.equal(sim.old, before[1])
    # and the legal edge: a launch that holds no sample writes no row
    assert _raw_rec(sim, log, steps=4, every=9, phase=5, row0=7) == (0, 0)
    sim.synchronize()
    assert (log == FILL).all() and not torch.equal(sim.old, before[1])
    e.set_watch(None)
    assert e.watch_count == 0 and _raw_rec(sim, log)[0] == E_STATE
    sim.close()


def test_sim_level_refusals(native_built):
    sc = scenes.scene_c2(n=1000)
    two_kernel = ClosedLoopSim(sc, fused=False)
    with pytest.raises(ValueError, match="fused"):
        two_kernel.record([0])
    two_kernel.close()
    sim = ClosedLoopSim(sc)
    for bad in ([1000], [3, 3], []):
        with pytest.raises(ValueError):
            sim.record(bad)
    assert sim.recorder is None and sim.engine.watch_count == 0
    rec = sim.record([7, 3], every=2, rows=5)
    rec.log.fill_(FILL)
    start = sim.state()
    with pytest.raises(ValueError, match="graph"):
        sim.run(128, graph_steps=64)
    with pytest.raises(ValueError, match="rows"):
        sim.run_resident(12, chunk=4)                            # would need 6 rows: refused as a whole, before the first launch
    with pytest.raises(ValueError, match="rows"):
        sim.run_eager(12)
    assert sim.steps_done == 0 and rec.rows_written == 0 and np.array_equal(sim.state(), start) and (rec.log == FILL).all()
    sim.run(10, graph_steps=0)                                   # no replays: eager stepping, which records
    assert list(rec.steps()) == [2, 4, 6, 8, 10]
    sim.close()
