"""The peak tension of every tether link on the device (hydro_step_fused_tiled_multi_peak): the record one launch of seven steps
leaves is, bit for bit, the host's fold (LinkTensions.fold) of the probe's tensions (hydro_tether_wrench, layer by layer) on the
states the seven steps start from; 7 = 7 x 1 = (2, 5); both ends of a link hold the same bits; a pre-seeded record comes out as
the compare-and-select says; nothing feeds back - state, prev_out, energy, log and extremes are the net entry's bits with every
option on, in the KE, NT and Warp instantiations, and a NULL record IS the net entry; padding lanes and guard bands stay;
refusals launch nothing; ClosedLoopSim's three runners and a graph replay leave the same record; the hanging chains' peaks carry
the submerged weight below each link; the example.

Sizes and population: n = 200, 321 and 322 and the four-layer net of tests/tether_net_population.py, as tests/test_tether_net_gpu.py;
tests/test_link_tensions.py shows by the fp64 reference that its peaks fall on first, interior and last steps in two layers.
No tolerance appears below but one: every comparison is of bits, and the hanging chains' bound is the fp64 run's own residual
(0.0362 N)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from silver2_isaacsim_amd.tether import LinkTensions, Tether, TetherNet
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from resident_harness import (_buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, _from, _guarded, _ke, NAN, S_A, S_C, S_IN, S_M, S_OUT, S_PV,
                              S_PVO, _same, _same_bits, _tiled, _unguard, _untouched)
from tether_net_population import hanging_chain, hanging_constants, HANG_STEPS, LINK, net_for, net_population, SIZES

pytestmark = pytest.mark.gpu
S_E = 8 * 64 + 36                                                 # the extremes record's tile stride in the guard tests
FP64_RESIDUAL = 0.0362                                            # N: |T - weight| of the fp64 run of the hanging chain after 3600 steps


def S_N(layers):
    """The net's tile stride in the guard tests."""
    return 448 * layers + 44


def S_P(layers):
    """The tile stride of the record of the link tensions in the guard tests."""
    return 64 * layers + 52


@pytest.fixture(scope="module")
def pop(bed_pop, hold_pop):
    """The bodies, net and mooring lines of tests/test_tether_net_gpu.py."""
    st, pv, params, applied, ctl = bed_pop
    more = hold_pop
    cat = lambda a, b: np.concatenate([a, b[321:322]])  # noqa: E731
    applied, ctl = cat(applied, more[3]), cat(ctl, more[4])
    params = {k: cat(params[k], more[2][k]) for k in params}
    st, pv, pr, net, groups = net_population()
    assert np.array_equal(pr, params["f32"])
    moor = np.concatenate([line_population(st[:321], params["f32"][:321]), np.zeros((1, 9), np.float32)])
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, net=net, groups=groups, moor=moor)


def step_peak(eng, cur, old, n, steps, *, net, layers, peaks, step0=0, applied=None, frame="world", control=None, mooring=None, extremes=None,
              implicit=False, ke=None, **kw):
    """One launch of the new entry through the engine; (state, prev_out)."""
    eng.step_fused_tiled_multi_peak(cur, old, n, DT, steps, step0, net, layers, peaks, extremes, mooring, control, applied, frame, implicit_drag=implicit,
                                    ke_out=ke, **kw)
    return old, cur[:, 7:13]


def step_net(eng, cur, old, n, steps, *, net, layers, step0=0, applied=None, frame="world", control=None, mooring=None, extremes=None, implicit=False,
             ke=None, **kw):
    """One launch of the net entry through the engine; (state, prev_out)."""
    eng.step_fused_tiled_multi_net(cur, old, n, DT, steps, step0, net, layers, extremes, mooring, control, applied, frame, implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


def raw_peak(eng, n, state, prev, out, pvo, *, layers, s_tether, tether, peaks, s_peaks, steps=1, step0=0, implicit=0, log=None, fields=13, frame=0,
             applied=None, control=None, mooring=None, extremes=None):
    """hydro_step_fused_tiled_multi_peak with the guard tests' strides; (rc, rows_written from the sentinel -7)."""
    ptr = lambda b: b.data_ptr() if hasattr(b, "data_ptr") else b  # noqa: E731
    written = ctypes.c_int64(-7)
    rc = eng._lib.hydro_step_fused_tiled_multi_peak(
        eng._h, n, ptr(state), S_IN, ptr(prev), S_PV, DT, steps, ptr(out), S_OUT, ptr(pvo), S_PVO,
        int(implicit), 1, None, ptr(log), 8, 4, fields, 1, 1, 0, ctypes.byref(written),
        ptr(applied), S_A, frame, ptr(control), S_C, ptr(mooring), S_M, ptr(extremes), S_E, ptr(tether), s_tether, layers, ptr(peaks), s_peaks, step0,
        eng._stream(None))
    return rc, written.value


def _tensions(eng, cur, net, n, layers):
    """(L, n) the probe's tension of each body's line in each layer on the tiled state `cur`."""
    _, t = eng.tether_net_wrench(cur, net, n, layers)
    return np.stack([_from(x, n)[:, 0] for x in t])


def _partners(net, n, l):
    return 64 * (np.arange(n) // 64) + net[:, 7 * l + 6].astype(np.int64)


# ---- 1. bits against the probe ---------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_the_record_is_the_fold_of_the_probes_tensions(coeff, implicit, pop, native_built):
    """Seven single steps of the NET entry, the probe called on the state in front of each; the host folds the seven (L, n) tension
    outputs.  One launch of seven steps of the new entry from an all-zero record leaves that record bit for bit, and so do
    7 x 1 and (2, 5) launches; the states are the net entry's; both ends of every link hold the same bits; a record seeded with a
    huge value, a NaN and +0 in slots whose lines pull comes out as the fold of the same samples into that seed."""
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        rec = net_for(pop["net"], n)
        net = _tiled(rec)
        cur, old = _buffers(st, pv, n)
        samples = []
        for i in range(7):
            samples.append(_tensions(eng, cur, net, n, 4))
            step_net(eng, cur, old, n, 1, step0=i, net=net, layers=4, implicit=implicit)
            cur, old = old, cur
        torch.cuda.synchronize()
        final = cur.clone()
        samples = np.stack(samples)
        assert samples.shape == (7, 4, n) and not np.isnan(samples).any() and not np.signbit(samples).any()
        want = LinkTensions.fold(samples)
        # the population does what tests/test_link_tensions.py shows by the reference: neither the first nor the last sample is the peak
        for l in (0, 1):
            assert (want[:, l] != samples[0, l]).sum() >= 8 and (want[:, l] != samples[6, l]).sum() >= 8 and (want[:, l] > 0).sum() >= n // 5, (n, l)
        assert (want[:, 2] > 0).sum() == 2 and not want[:, 3].any()

        def run(chunks, seed=None):
            cur, old = _buffers(st, pv, n)
            peaks = eng.alloc_tiled(4, n) if seed is None else _tiled(seed)
            done = 0
            for k in chunks:
                step_peak(eng, cur, old, n, k, step0=done, net=net, layers=4, peaks=peaks, implicit=implicit)
                cur, old = old, cur
                done += k
            torch.cuda.synchronize()
            return cur, peaks
        state, peaks = run([7])
        got = _from(peaks, n)
        assert _same(got, want), (n, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert _same_bits(state, final)                            # nothing feeds back
        assert not peaks.reshape(-1, 4, 64)[-1, :, n % 64 or 64:].any()       # the padding lanes of the last tile
        for chunks in ([1] * 7, [2, 5]):
            other_state, other = run(chunks)
            assert _same_bits(other, peaks) and _same_bits(other_state, final), (n, chunks)
        for l in range(4):
            assert _same(np.ascontiguousarray(got[:, l]), np.ascontiguousarray(got[_partners(rec, n, l), l])), (n, l)
        # a seed: among the bodies with a peak in layers 0 and 1, a huge value, a NaN and +0 in known slots
        seed = np.zeros((n, 4), np.float32)
        a, b, c = np.flatnonzero(want[:, 0] > 0)[[0, 3, 5]]
        d, e = np.flatnonzero(want[:, 1] > 0)[[1, 2]]
        seed[a, 0], seed[b, 0], seed[d, 1], seed[e, 1] = 1e30, np.nan, np.float32(3e38), want[e, 1]
        seed[4, 3] = 2.5                                         # a slot nobody writes keeps what it held
        _, seeded = run([7], seed)
        seeded = _from(seeded, n)
        assert _same(seeded, LinkTensions.fold(samples, seed)), n
        assert seeded[a, 0] == np.float32(1e30) and seeded.view(np.uint32)[b, 0] == seed.view(np.uint32)[b, 0] and seeded[c, 0] == want[c, 0] > 0
        assert seeded[d, 1] == np.float32(3e38) and seeded[e, 1] == want[e, 1] and seeded[4, 3] == 2.5
        eng.close()


# ---- 2. nothing feeds back ---------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
def test_nothing_feeds_back_with_every_option_on(coeff, semantics, implicit, pop, native_built):
    """Applied wrench, pose hold, a two-wave sea, bed, mooring lines, extremes and the recorder, with and without the kinetic
    energy (KE), streaming (NT) and in both semantics (Warp): state, prev_out, energy, log and extremes record of the new entry
    are bit for bit the net entry's, a NULL record IS the net entry, and the record equals the one the temporal launch without
    energy leaves - which is the fold of the probe's tensions on the recorded states' predecessors."""
    st, pv = pop["st"], pop["pv"]
    sea = SeaState(SEA.current).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])
    assert len(sea.waves) == 2
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_sea(sea)
        eng.set_seabed(BED)
        watched = sorted({b for b in (0, 5, 8, 11, 40, 63, 64, 80, 130, n - 1) if b < n})
        eng.set_watch(watched)
        net, m9, a, c17 = _tiled(net_for(pop["net"], n)), _tiled(pop["moor"][:n]), _tiled(pop["applied"][:n]), _tiled(pop["ctl"][:n])

        def run(launch, steps=7, ke=None, start=None, step0=5):
            cur, old = _buffers(st, pv, n) if start is None else start
            log = torch.full((8, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            ext = eng.extremes_reset(eng.alloc_tiled(8, n), n)
            state, prev = launch(eng, cur, old, n, steps, step0=step0, net=net, layers=4, extremes=ext, mooring=m9, control=c17, applied=a, implicit=implicit,
                                 ke=ke, log=log)
            torch.cuda.synchronize()
            return [state, prev, log, ext] + ([ke] if ke is not None else [])
        with_record = lambda peaks: lambda *args, **kw: step_peak(*args, peaks=peaks, **kw)  # noqa: E731
        records = []
        for nt in (0, 1):
            eng.set_tuning(0, 0, nt)
            for energy in (False, True):
                want = run(step_net, ke=_ke() if energy else None)
                peaks = eng.alloc_tiled(4, n)
                got = run(with_record(peaks), ke=_ke() if energy else None)
                assert all(_same_bits(x, y) for x, y in zip(got, want)), (n, nt, energy)
                null = run(with_record(None), ke=_ke() if energy else None)
                assert all(_same_bits(x, y) for x, y in zip(null, want)), (n, nt, energy)
                records.append(peaks)
        eng.set_tuning(0, 0, 0)
        assert all(_same_bits(r, records[0]) for r in records[1:]) and (_from(records[0], n) > 0).sum() >= n // 4, n
        # the fold of the probe's tensions along the same seven steps, taken one at a time through the net entry
        cur, old = _buffers(st, pv, n)
        samples = []
        for i in range(7):
            samples.append(_tensions(eng, cur, net, n, 4))
            cur, old = run(step_net, steps=1, start=(cur, old), step0=5 + i)[0], cur
        assert _same(_from(records[0], n), LinkTensions.fold(np.stack(samples))), n
        eng.close()


# ---- 3. guards and refusals through the raw C ABI -----------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_strides_and_nan_guards(coeff, implicit, pop, native_built):
    """n = 200, three layers, the record at a tile stride of 64 L + 52 with NaN in the stride padding and in the lanes past body
    n: the bodies' slots are those of the tightly packed launch, no sentinel is overwritten, every input is untouched; and a launch
    with a NULL record (the net entry's) leaves a record lying by untouched."""
    st, pv = pop["st"], pop["pv"]
    n, tiles, L = 200, 4, 3
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    rec = net_for(pop["net"], n, L)
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m9, t21 = _guarded(pop["moor"][:n], S_M), _guarded(rec, S_N(L))
    empty = np.tile(np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0], np.float32), (n, 1))
    e8, p3 = _guarded(empty, S_E), _guarded(np.zeros((n, L), np.float32), S_P(L))
    before = [b.cpu().numpy() for b in (state, prev, a, c17, m9, t21)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    args = dict(layers=L, s_tether=S_N(L), tether=t21.data_ptr(), steps=3, step0=11, implicit=implicit, applied=a.data_ptr(), control=c17.data_ptr(),
                mooring=m9.data_ptr(), extremes=e8.data_ptr())
    rc, _ = raw_peak(eng, n, state, prev, out, pvo, peaks=p3.data_ptr(), s_peaks=S_P(L), **args)
    eng._check(rc)
    torch.cuda.synchronize()
    got, rest = _unguard(p3, n, L, S_P(L))
    assert np.isnan(rest).all(), "a padding lane or a guard band of the record was written"
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17, m9, t21), before))
    final = _unguard(out, n, 13, S_OUT)[0]
    peaks = eng.alloc_tiled(L, n)
    cur, old = _buffers(st, pv, n)
    want_state, _ = step_peak(eng, cur, old, n, 3, step0=11, net=_tiled(rec), layers=L, peaks=peaks, extremes=eng.extremes_reset(eng.alloc_tiled(8, n), n),
                              mooring=_tiled(pop["moor"][:n]), control=_tiled(pop["ctl"][:n]), applied=_tiled(pop["applied"][:n]), implicit=implicit)
    torch.cuda.synchronize()
    assert _same(got, _from(peaks, n)) and (got > 0).sum() >= n // 4 and _same(final, _from(want_state, n))
    # the net entry's launch never touches a record
    held = p3.cpu().numpy()
    rc, _ = raw_peak(eng, n, state, prev, out, pvo, peaks=None, s_peaks=S_P(L), **args)
    eng._check(rc)
    torch.cuda.synchronize()
    assert _untouched(p3, held) and _same(_unguard(out, n, 13, S_OUT)[0], final)
    eng.close()


def test_refusals_launch_nothing(pop, native_built):
    """After the net entry's own refusals: a record without a net, a stride of 64 L - 64, a misaligned record, the record over
    state_out, over the last layer of the net, over the extremes record, over the state and over the log."""
    n, L = 322, 3
    tiles, s_n, s_p = (n + 63) // 64, S_N(3), S_P(3)
    st, pv = pop["st"], pop["pv"]
    eng = _engine(n, pop["params"]["f32"], "f32")
    eng.set_watch([0, 5])
    state, prev = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV)
    net = _guarded(net_for(pop["net"], n, 3), s_n)
    before = net.cpu().numpy()
    e8 = torch.full((tiles * S_E,), NAN, device=DEV)
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 13, 8), NAN, device=DEV)
    p3 = torch.full((tiles * s_p,), NAN, device=DEV)
    E_ARG = -1
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    call = lambda **kw: raw_peak(eng, n, state, prev, out, pvo, **{**dict(layers=L, s_tether=s_n, tether=net, peaks=p3, s_peaks=s_p, extremes=e8, log=log), **kw})  # noqa: E731
    p = p3.data_ptr()
    assert call(tether=None) == (E_ARG, -7) and "tether_peaks without a tether net" in last()
    assert call(layers=5) == (E_ARG, -7) and "tether_layers" in last()                              # the net entry's own come first
    assert call(s_peaks=64 * L - 64) == (E_ARG, -7) and "stride" in last()
    assert call(peaks=p + 4) == (E_ARG, -7) and "aligned" in last()
    over = "tether_peaks must not overlap"
    assert call(peaks=out) == (E_ARG, -7) and over in last()
    assert call(peaks=out.data_ptr() + 4 * ((tiles - 1) * S_OUT + 12 * 64)) == (E_ARG, -7) and over in last()      # the last field of the last tile
    assert call(peaks=net.data_ptr() + 4 * ((tiles - 1) * s_n + 448 * (L - 1) + 6 * 64), s_peaks=64 * L) == (E_ARG, -7) and over in last()   # the last layer of the net
    assert call(peaks=e8) == (E_ARG, -7) and over in last()
    assert call(peaks=state) == (E_ARG, -7) and over in last()
    assert call(peaks=log, s_peaks=64 * L) == (E_ARG, -7) and over in last()
    torch.cuda.synchronize()
    assert all(torch.isnan(b).all() for b in (out, pvo, log, e8, p3)) and _untouched(net, before)
    eng.close()


# ---- 4. ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def _scene():
    """Config 2's bodies (n = 322) and the net of tests/test_tether_net_gpu.py's sim tests: in every tile chains of five consecutive
    bodies, each link a tenth shorter than the distance between its fairleads, constants from for_chain; a bridle on the first link
    of every chain of tile 0 (three layers).  And pairs (2 i, 2 i + 1) for set_tether, each a tenth shorter than its distance."""
    sc = scenes.scene_c2(n=322)
    m = sc.params[:, 10].astype(np.float64)
    fa, fb = np.array([0.05, 0.0, -0.05]), np.array([0.0, 0.05, 0.05])
    links, k, c = [], [], []
    for t in range(6):
        for j in range(12):
            bodies = 64 * t + 5 * j + np.arange(5)
            if j % 4 == 3 or bodies[-1] >= 322:
                continue
            kj, cj = TetherNet.for_chain(m[bodies], sc.dt)
            for a, b in zip(bodies[:-1], bodies[1:]):
                links.append((a, b))
                k.append(0.5 * kj)
                c.append(0.5 * cj)
            if t == 0:
                links.append((bodies[0], bodies[1]))
                k.append(0.5 * kj)
                c.append(0.5 * cj)
    links = np.array(links)
    pos = sc.state[:, 0:3].astype(np.float64)
    d = np.linalg.norm(pos[links[:, 1]] + fb - pos[links[:, 0]] - fa, axis=1)               # (unit quaternions at the start)
    net = dict(links=links, fairlead_a=fa, fairlead_b=fb, length=0.9 * d, stiffness=np.array(k), damping=np.array(c))
    a = np.arange(0, 300, 2)                                                                 # (bodies 300 .. 321 stay untied)
    pk, pc = Tether.for_pair(m[a], m[a + 1], sc.dt)
    pairs = dict(pairs=np.stack([a, a + 1], axis=1), length=0.9 * np.linalg.norm(pos[a + 1] - pos[a], axis=1), stiffness=pk, damping=pc)
    return sc, net, pairs


@pytest.mark.parametrize("tethers", ["net", "set_tether"])
def test_sim_runners_and_a_graph_replay_leave_the_same_record(tethers, native_built):
    sc, net, pairs = _scene()
    tie = (lambda s: s.set_tether_net(**net)) if tethers == "net" else (lambda s: s.set_tether(**pairs))
    layers, m = (3, len(net["links"])) if tethers == "net" else (1, len(pairs["pairs"]))
    records, finals = {}, {}
    for name, go in (("eager", lambda s: s.run_eager(64)), ("resident", lambda s: s.run_resident(64)), ("chunks", lambda s: s.run_resident(64, chunk=24)),
                     ("graph", lambda s: s.run(64, graph_steps=32))):
        sim = ClosedLoopSim(sc, implicit_drag=True)
        tie(sim)
        view = sim.track_link_tensions()
        assert view is sim.link_tensions and tuple(view.buffer.shape) == (6, layers, 64)
        go(sim)
        assert name != "graph" or sim._graph is not None
        records[name], finals[name] = view.record(), sim.state()
        assert records[name].shape == (322, layers) and view.peak().shape == (m,)
        if name == "resident":
            # the view: both ends of a link read the same, peak() is the caller's order; reset() empties, and the record accumulates again
            peak = view.peak()
            assert (peak > 0).mean() > 0.9 and _same(peak, np.ascontiguousarray(records[name][view.links[:, 1], view.layer]))
            untied = ~np.isin(np.arange(322), view.links.reshape(-1))
            assert untied.any() and not records[name][untied].any()
            view.reset()
            assert not view.record().any()
            sim.run_resident(8)
            assert (view.peak() > 0).any()
            # clear_link_tensions: the parent's calls again, and the record keeps its contents
            kept = view.record()
            sim.clear_link_tensions()
            assert sim.link_tensions is None
            sim.run_resident(24)
            assert _same(view.record(), kept)
            parent = ClosedLoopSim(sc, implicit_drag=True)
            tie(parent)
            parent.run_resident(64 + 8 + 24)
            assert _same(sim.state(), parent.state())              # tracking never fed back, and the steps after it are the parent's
            parent.close()
        sim.close()
    for name in ("resident", "chunks", "graph"):
        assert _same(records["eager"], records[name]) and _same(finals["eager"], finals[name]), name
    plain = ClosedLoopSim(sc, implicit_drag=True)
    with pytest.raises(ValueError, match="no tethers to track"):
        plain.track_link_tensions()
    tie(plain)
    plain.track_link_tensions()
    plain.set_sea(SEA)
    with pytest.raises(ValueError, match="graph replays"):          # a net plus waves in a replay stays refused
        plain.run(64, graph_steps=32)
    plain.close()


# ---- 5. physics: the hanging chains ------------------------------------------------------------------------------------------------------
def test_the_hanging_chains_peaks_carry_the_weight_below_each_link(native_built):
    """64 copies of tether_net_population.hanging_chain (the layout of tests/test_tether_net_gpu.py), HANG_STEPS steps resident with
    the link tensions tracked: every link's peak is at least its tension at the end (the probe on the final state) and at least
    the submerged weight below it minus the fp64 run's own residual, 0.0362 N; resident and eager leave the same bits."""
    st5, pv5, pr5, sc, dt, hang = hanging_chain()
    rng = np.random.default_rng(9)
    n = 340
    chains = []
    for t in range(6):
        lanes = np.arange(60).reshape(12, 5) if t % 2 == 0 or t == 5 else np.concatenate([np.arange(12)[:, None], 12 + rng.permutation(48).reshape(12, 4)], axis=1)
        chains += [64 * t + row for row in lanes[:4 if t == 5 else 12]]
    chains = np.array(chains)
    assert chains.shape == (64, 5) and chains.max() < n and len(np.unique(chains)) == 320
    st, pv, pr = np.tile(st5[0], (n, 1)), np.tile(pv5[0], (n, 1)), np.tile(pr5[0], (n, 1))          # (spare lanes: buoys)
    for i in range(5):
        st[chains[:, i]], pv[chains[:, i]], pr[chains[:, i]] = st5[i], pv5[i], pr5[i]
    spot = np.arange(n)
    st[:, 0], st[:, 1] = 20.0 * (spot % 20), 20.0 * (spot // 20)
    for i in range(1, 5):
        st[chains[:, i], 0:2] = st[chains[:, 0], 0:2]
    scene = scenes.Scene("hanging chains", st, pv, pr, dt=dt, rho=sc.rho, g=sc.g)
    k, c = hanging_constants(pr5, dt)
    links = np.concatenate([np.stack([chains[:, i], chains[:, i + 1]], axis=1) for i in range(4)])
    lines = dict(links=links, length=LINK, stiffness=k, damping=c, layer=np.repeat([0, 1, 0, 1], 64))
    sim, eager = ClosedLoopSim(scene, implicit_drag=True), ClosedLoopSim(scene, implicit_drag=True)
    for s in (sim, eager):
        s.set_tether_net(**lines)
        s.track_link_tensions()
    sim.run_resident(96, chunk=32)
    eager.run_eager(96)
    assert _same(sim.link_tensions.record(), eager.link_tensions.record()) and _same(sim.state(), eager.state())
    sim.run_resident(HANG_STEPS - 96, chunk=64)
    peak = sim.link_tensions.peak().astype(np.float64).reshape(4, 64)
    _, t = sim.engine.tether_net_wrench(sim.cur, sim.tether_net, n, 2)
    at_end = np.stack([_from(x, n)[:, 0] for x in t]).T[links[:, 0], lines["layer"]].astype(np.float64).reshape(4, 64)
    print("[hanging chains, link tensions] peak " + "  ".join(f"{a:.2f} .. {b:.2f}" for a, b in zip(peak.min(axis=1), peak.max(axis=1)))
          + " N  at the end " + "  ".join(f"{a:.2f} .. {b:.2f}" for a, b in zip(at_end.min(axis=1), at_end.max(axis=1)))
          + " N  weight below " + " ".join(f"{w:.2f}" for w in hang) + f" N  smallest peak - weight {(peak - hang[:, None]).min():.4f} N (bound -{FP64_RESIDUAL} N)")
    assert (at_end > 0).all() and (peak >= at_end).all()
    assert (peak >= hang[:, None] - FP64_RESIDUAL).all()
    for x in (sim, eager):
        x.close()


def test_cable_design_loads_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "cable_design_loads.py"), "--steps", "600"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    assert "peak tension" in res.stdout
