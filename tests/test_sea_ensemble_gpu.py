"""Sea ensembles on the device (hydro_set_sea_ensemble, hydro_sea_ensemble_sample, hydro_step_fused_tiled_multi_ens).  The yardstick
is the identity of include/hydro.h ("Sea ensemble"): bit for bit, a body of member m takes the step it takes in
hydro_step_fused_tiled_multi_stat under hydro_set_sea_spectrum(member m).  So for every member the PARENT's entry is run over the
whole population under that member's spectrum, the expectation takes block m of every output from run m, and the _ens launch must
equal it in state_out, prev_out, the log rows, the extremes, the link tensions and every word of the statistics record - no second
oracle and no tolerance.  Before the comparison the parent's runs themselves must show that any two members move at least 9 in 10 of
the bodies differently after one step, and some body of every tile (tests/test_sea_ensemble.py shows the same on the fp64 closed
loop): "member 0 for everyone" or "the neighbour's table" then fails on every tile.

Shapes: n = 65 (one live lane in tile 1, which belongs to member 1), 200 and 321 (2, 4 and 6 tiles; a block of 256 is four tiles) at
tiles_per_sea = 1 (four members inside one block); n = 321 at tiles_per_sea = 2 (three members, a block boundary inside the
ensemble, the last member partial) and 4 (member 1 a partial block).  f32 and f16, explicit and implicit, 1 and 7 steps, 11 and 64
components (11 takes the component loops' remainder trips).  The population, the spread and the net are those of
tests/test_statistics_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sea_ensemble_harness as seh
import statistics_reference as sx
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.extremes import Extremes
from silver2_isaacsim_amd.mooring import MooringSpread
from silver2_isaacsim_amd.sea import SeaEnsemble, SeaSpectrum, SeaState, jonswap_ensemble
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from mooring_spread_population import spread_population
from resident_harness import (_buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, _from, _guarded, _in_one_allocation, _ke, NAN, S_A, S_C, S_IN, S_OUT, S_PV,
                              S_PVO, _same_bits, _tiled, _unguard, _untouched, VIEW_STEPS, _watched)
from tether_net_population import net_for, net_population

pytestmark = pytest.mark.gpu
CASES = ((65, 1), (200, 1), (321, 1), (321, 2), (321, 4))         # (n, tiles_per_sea)
STEPS = (1, 7)
WAVES = pytest.mark.parametrize("waves", [11, 64])
S_E, S_T2, S_P2, S_SP3 = 8 * 64 + 36, 448 * 2 + 44, 64 * 2 + 20, 576 * 3 + 52      # extremes, a two-layer net, its link tensions, a spread of three
E_ARG, E_STATE = -1, -5


@pytest.fixture(scope="module")
def pop(bed_pop):
    """tests/test_statistics_gpu.py's population: 321 bodies over the bed with the designed spread and the tether net."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, _ = net_population()
    st, pv = st[:321], pv[:321]
    spread = spread_population(st, params["f32"], line_population(st, params["f32"]))
    return dict(st=st, pv=pv, params=params, applied=applied, ctl=ctl, spread=spread, net=net)


def _record(eng, n):
    """A fresh record: NaN everywhere, then reset - so the reset has written every live word."""
    return eng.statistics_reset(torch.full((eng.tiles(n), nat.STAT_FIELDS, 64), NAN, dtype=torch.float32, device=DEV), n)


def _levels_for(st, n):
    """(n, 2) fp32 levels: z near its initial value - some above, some below, some equal - and the tension against +0."""
    rng = np.random.default_rng(n)
    lev = np.stack([st[:n, 2], np.zeros(n, np.float32)], axis=1).astype(np.float32)
    lev[:, 0] += rng.choice(np.array([-1e-3, 0.0, 1e-3], np.float32), size=n)
    return lev


def _water(eng, water):
    """The engine's water: None, a SeaState, a SeaSpectrum or a SeaEnsemble - whatever was set before is cleared first."""
    eng.set_sea(None)
    eng.set_sea_spectrum(None)
    eng.set_sea_ensemble(None)
    if isinstance(water, SeaEnsemble):
        eng.set_sea_ensemble(water)
    elif isinstance(water, SeaSpectrum):
        eng.set_sea_spectrum(water)
    elif water is not None:
        eng.set_sea(water)


def _everything(eng, entry, pop, n, steps, step0, implicit, ke=None, bare=False, record=True, chunks=None):
    """A launch (or, `chunks`, several) of `entry` ("ens" / "stat") with the spread of three, the two-layer net with its link tensions,
    extremes, pose hold, a body-frame applied wrench, a log of three watched bodies and the statistics - or, bare, with nothing but
    (`record`) the statistics.  Returns every output by name."""
    cur, old = _buffers(pop["st"], pop["pv"], n)
    kw, out = {}, {}
    if record:
        out["record"] = _record(eng, n)
        kw.update(statistics=out["record"], levels=_tiled(_levels_for(pop["st"], n)), channels=(2, 6))
    if not bare:
        watched = _watched(n, (0, 63, 64))
        eng.set_watch(watched)
        out["log"] = torch.full((steps, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
        out["extremes"], out["peaks"] = eng.extremes_reset(eng.alloc_tiled(8, n), n), eng.alloc_tiled(2, n)
        kw.update(spread=_tiled(pop["spread"][:n, 0:27]), layers=3, tether=_tiled(net_for(pop["net"], n, 2)), net_layers=2, peaks=out["peaks"],
                  extremes=out["extremes"], applied=_tiled(pop["applied"][:n]), control=_tiled(pop["ctl"][:n]), frame="body")
    done, row0 = 0, 0
    for k in (chunks or [steps]):
        more = dict(log=out["log"], every=1, phase=1, row0=row0) if not bare else {}
        seh.launch(eng, cur, old, n, k, step0=step0 + done, implicit=implicit, ke=ke, entry=entry, **kw, **more)
        cur, old = old, cur
        done, row0 = done + k, row0 + k
    torch.cuda.synchronize()
    out["state"], out["prev"] = cur.clone(), old[:, 7:13].clone()
    if ke is not None:
        out["ke"] = ke
    return out


def _same_or_nan(a, b):
    i = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(((a.contiguous().view(i) == b.contiguous().view(i)) | (torch.isnan(a) & torch.isnan(b))).all())


def _expected(runs, n, tiles_per_sea):
    """Block m of every output from the parent's run under member m: tiled outputs (the record among them) tile by tile, the log by
    the tile of each column's watched body.  The energy pair is a sum over all bodies and has no such composition (see 5.)."""
    want = {}
    for name, first in runs[0].items():
        if name == "ke":
            continue
        x = first.clone()
        if name == "log":
            for j, b in enumerate(_watched(n, (0, 63, 64))):
                x[:, :, j] = runs[(b // 64) // tiles_per_sea][name][:, :, j]
        else:
            for t in range(x.shape[0]):
                x[t] = runs[t // tiles_per_sea][name][t]
        want[name] = x
    return want


def _equal(got, want, n):
    for name, x in want.items():
        if name == "record":
            if not sx.same_record(stx.unpack(got[name].cpu().numpy(), n), stx.unpack(x.cpu().numpy(), n)):
                return name
        elif not _same_or_nan(got[name], x):
            return name
    return None


def _member_runs(eng, members, pop, n, steps, implicit, bare, step0=5, **kw):
    runs = []
    for m in members:
        _water(eng, m)
        runs.append(_everything(eng, "stat", pop, n, steps, step0, implicit, bare=bare, **kw))
    return runs


# ---- 1, 2. the identity, and the condition that makes it mean something -------------------------------------------------------------------
@COEFFS
@DRAG
@WAVES
def test_every_block_takes_its_members_step_bit_for_bit(waves, coeff, implicit, pop, native_built):
    members = seh.members(waves)
    for n in sorted({n for n, _ in CASES}):
        tiles = (n + 63) // 64
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_seabed(BED)
        for bare in (False, True):
            for steps in STEPS:
                runs = _member_runs(eng, members[:tiles], pop, n, steps, implicit, bare)
                if steps == 1:
                    # the condition, on the parent's runs alone: any two members move nearly every body differently, in every tile
                    fraction, every_tile = seh.apart([_from(r["state"], n) for r in runs], n)
                    assert fraction >= 0.9 and every_tile, (n, bare, fraction, every_tile)
                for tps in (t for m, t in CASES if m == n):
                    ens = seh.ensemble(waves, n, tps)
                    assert [m.waves for m in ens.members] == [m.waves for m in members[:ens.count]]
                    _water(eng, ens)
                    got = _everything(eng, "ens", pop, n, steps, 5, implicit, bare=bare)
                    assert _equal(got, _expected(runs, n, tps), n) is None, (n, tps, bare, steps, _equal(got, _expected(runs, n, tps), n))
                    rec = stx.unpack(got["record"].cpu().numpy(), n)
                    assert (rec["n"] == steps).all()
                    # without a record: the family without statistics, the same bits in everything else
                    plain = _everything(eng, "ens", pop, n, steps, 5, implicit, bare=bare, record=False)
                    assert all(_same_or_nan(plain[k], got[k]) for k in plain), (n, tps, bare, steps)
        eng.close()


# ---- 3. degeneracy ---------------------------------------------------------------------------------------------------------------------------
def test_without_an_ensemble_the_launch_is_the_stat_entrys_with_each_option_alone(pop, native_built):
    """The ladder row: n = 65, 2 steps, f32, explicit, with the kinetic energy - each option alone, and none, with and without a record,
    in still water, in a regular sea and under a spectrum."""
    n, steps, step0 = 65, 2, 3
    st, pv = pop["st"], pop["pv"]
    lev = _tiled(_levels_for(st, n))
    spec = seh.members(11)[2]
    for option in (None, "log", "applied", "control", "sea", "spectrum", "seabed", "spread", "extremes", "net", "peaks"):
        eng = _engine(n, pop["params"]["f32"], "f32")
        eng.set_watch([0, 5, 63, 64])
        _water(eng, SEA if option == "sea" else spec if option == "spectrum" else None)
        eng.set_seabed(BED if option == "seabed" else None)
        layers = 2 if option in ("net", "peaks") else 1

        def run(entry, with_record):
            cur, old = _buffers(st, pv, n)
            ke = _ke()
            log = torch.full((steps, 19, 4), NAN, dtype=torch.float32, device=DEV) if option == "log" else None
            extremes = eng.extremes_reset(eng.alloc_tiled(8, n), n) if option == "extremes" else None
            peaks = eng.alloc_tiled(layers, n) if option == "peaks" else None
            record = _record(eng, n) if with_record else None
            kw = dict(step0=step0, spread=_tiled(pop["spread"][:n, 0:27]) if option == "spread" else None, layers=3,
                      tether=_tiled(net_for(pop["net"], n, layers)) if option in ("net", "peaks") else None, net_layers=layers, peaks=peaks,
                      extremes=extremes, applied=_tiled(pop["applied"][:n]) if option == "applied" else None,
                      control=_tiled(pop["ctl"][:n]) if option == "control" else None, frame="body", ke=ke,
                      statistics=record, levels=lev if with_record else None, channels=(2, 6))
            if log is not None:
                kw.update(log=log, every=1, phase=1, row0=0)
            state, prev = seh.launch(eng, cur, old, n, steps, entry=entry, **kw)
            torch.cuda.synchronize()
            return [state, prev, ke] + [x for x in (log, extremes, peaks, record) if x is not None]
        for with_record in (False, True):
            want, got = run("stat", with_record), run("ens", with_record)
            assert len(got) == len(want) and all(_same_bits(x, y) for x, y in zip(got, want)), (option, with_record)
        eng.close()


@COEFFS
@DRAG
def test_one_member_over_everybody_is_the_stat_entry_under_that_spectrum(coeff, implicit, pop, native_built):
    for waves in (11, 64):
        member = seh.members(waves)[3]
        for n in (65, 321):
            eng = _engine(n, pop["params"][coeff], coeff)
            eng.set_seabed(BED)
            for bare in (False, True):
                _water(eng, member)
                want = _everything(eng, "stat", pop, n, 7, 5, implicit, bare=bare)
                for per_sea in (((n + 63) // 64) * 64, 1024):       # exactly the tiles of n, and a block that reaches far past n
                    _water(eng, SeaEnsemble([member], per_sea))
                    got = _everything(eng, "ens", pop, n, 7, 5, implicit, bare=bare)
                    assert _equal(got, want, n) is None, (waves, n, bare, per_sea)
            eng.close()


# ---- 4. stepping and launch variants ----------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    n = 321
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_seabed(BED)
    for tps in (1, 2):
        _water(eng, seh.ensemble(64, n, tps))
        for step0 in (0, 10 ** 6):
            whole = _everything(eng, "ens", pop, n, 7, step0, implicit)
            for chunks in ([1] * 7, [2, 5]):
                parts = _everything(eng, "ens", pop, n, 7, step0, implicit, chunks=chunks)
                assert _equal(parts, whole, n) is None, (tps, step0, chunks, _equal(parts, whole, n))
            assert (stx.unpack(whole["record"].cpu().numpy(), n)["n"] == 7).all()
    eng.close()


@COEFFS_SEMANTICS
def test_energy_and_non_temporal_instantiations(coeff, semantics, pop, native_built):
    """KE = true and NT = true (set_tuning(0, 0, 1)) in both semantics at 64 components with everything on, for both kernel families
    (with and without a record): the bits of the launch without sampling and of the temporal launch, which are the members' (the
    identity, once more, in these semantics); and - 5. - the energy pair against the fp64 host sum of the launch's own final state,
    at the gate of the resident tests (implicit drag, 1e-12)."""
    n, tps = 321, 1
    eng = _engine(n, pop["params"][coeff], coeff, semantics)
    eng.set_seabed(BED)
    eng.set_tuning(0, 0, 0)
    runs = _member_runs(eng, seh.members(64), pop, n, 7, True, False)
    _water(eng, seh.ensemble(64, n, tps))
    for record in (True, False):
        want = _everything(eng, "ens", pop, n, 7, 5, True, record=record)
        expected = _expected(runs, n, tps)
        assert _equal(want, {k: v for k, v in expected.items() if k in want}, n) is None
        got = _everything(eng, "ens", pop, n, 7, 5, True, ke=_ke(), record=record)
        assert _equal(got, want, n) is None
        state = _from(got["state"], n)
        assert np.isfinite(state).all()
        lin, rot = scenes.kinetic_energy_fp64(state, pop["params"][coeff][:n], rotational=True)
        pair = got["ke"].cpu().tolist()
        assert lin > 0 and rot > 0 and pair[0] == pytest.approx(lin, rel=1e-12) and pair[1] == pytest.approx(rot, rel=1e-12)
        eng.set_tuning(0, 0, 1)
        for ke in (None, _ke()):
            streamed = _everything(eng, "ens", pop, n, 7, 5, True, ke=ke, record=record)
            assert _equal(streamed, want, n) is None
            if ke is not None:
                assert _same_bits(streamed["ke"], got["ke"])
        eng.set_tuning(0, 0, 0)
    eng.close()


# ---- 6. the sample ----------------------------------------------------------------------------------------------------------------------------
@WAVES
def test_the_sample_is_the_members_sample_block_by_block(waves, pop, native_built):
    members = seh.members(waves)
    for n, tps in CASES:
        eng = _engine(n, pop["params"]["f32"], "f32")
        state = _tiled(pop["st"][:n])
        for step in VIEW_STEPS:
            per_member = []
            for m in members[:-(-((n + 63) // 64) // tps)]:
                _water(eng, m)
                per_member.append(eng.sea_spectrum_sample(state, n, step, DT).clone())
            _water(eng, seh.ensemble(waves, n, tps))
            out = torch.full((eng.tiles(n), 4, 64), NAN, dtype=torch.float32, device=DEV)
            assert eng.sea_ensemble_sample(state, n, step, DT, out=out) is out
            torch.cuda.synchronize()
            got, want = _from(out, n), np.concatenate([_from(per_member[t // tps], n)[64 * t:64 * (t + 1)] for t in range((n + 63) // 64)])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, tps, step)
            assert np.isnan(out.cpu().numpy().transpose(0, 2, 1).reshape(-1, 4)[n:]).all()               # the padding lanes are not written
        if tps == 1 and n > 64:
            a, b = per_member[0], per_member[1]
            assert not np.array_equal(_from(a, n)[64:], _from(b, n)[64:])                                # (and the members' water does differ)
        eng.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def _c_members(members):
    """(the ctypes array hydro_set_sea_ensemble takes, what keeps its rows alive)."""
    keep, arr = [], (nat.SeaSpectrum * max(len(members), 1))()
    for i, m in enumerate(members):
        rows = (nat.SeaWave * max(len(m.waves), 1))(*[nat.SeaWave(*w) for w in m.waves])
        keep.append(rows)
        arr[i].current[:] = list(m.current)
        arr[i].waves = len(m.waves)
        arr[i].wave = ctypes.cast(rows, ctypes.POINTER(nat.SeaWave)) if m.waves else None
    return arr, keep


def _raw_set(eng, members, count=None, bodies_per_sea=64):
    arr, keep = _c_members(members)
    return eng._lib.hydro_set_sea_ensemble(eng._h, arr, len(members) if count is None else count, bodies_per_sea)


def test_refusals_launch_nothing_write_nothing_and_keep_the_previous_ensemble(pop, native_built):
    n = 321
    tiles = (n + 63) // 64
    eng = _engine(n, pop["params"]["f32"], "f32")
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    members = seh.members(11)
    st, pv = pop["st"], pop["pv"]
    lev = _levels_for(st, n)
    state, prev, lv = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(lev, sx.S_LV)
    a, c17 = _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m27, net = _guarded(pop["spread"][:n, 0:27], S_SP3), _guarded(net_for(pop["net"], n, 2), S_T2)
    fresh = lambda stride: torch.full((tiles * stride,), NAN, device=DEV)  # noqa: E731
    e8, p2, out, pvo, record, water = fresh(S_E), fresh(S_P2), fresh(S_OUT), fresh(S_PVO), fresh(sx.S_ST), fresh(4 * 64 + 12)
    # one allocation in a fixed order (resident_harness._in_one_allocation): no call here hands a buffer over as another record, so no
    # claimed extent runs past its buffer - the arena only takes the allocator's placement out of the test, as in tests/test_statistics_gpu.py
    state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record, water = _in_one_allocation(state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record, water)
    everything = dict(applied=a, s_applied=S_A, control=c17, s_control=S_C, mooring=m27, s_mooring=S_SP3, layers=3, extremes=e8, s_extremes=S_E,
                      tether=net, s_tether=S_T2, net_layers=2, peaks=p2, s_peaks=S_P2, statistics=record, s_statistics=sx.S_ST, levels=lv, s_levels=sx.S_LV)

    def step(n_=n, **kw):
        args = dict(everything)
        args.update(kw)
        return seh.raw_ens(eng, n_, state, prev, out, pvo, **args)

    def sample(n_=n):
        return eng._lib.hydro_sea_ensemble_sample(eng._h, n_, state.data_ptr(), S_IN, 3, DT, water.data_ptr(), 4 * 64 + 12, eng._stream(None))
    # the sample without an ensemble
    assert sample() == E_STATE and "hydro_set_sea_ensemble" in last()
    # the setter's own refusals, with nothing set before: nothing becomes set
    assert _raw_set(eng, members, count=0) == E_ARG and "count" in last()
    assert _raw_set(eng, members, count=1025) == E_ARG and "count" in last()
    for bad in (0, 63, 96):
        assert _raw_set(eng, members, bodies_per_sea=bad) == E_ARG and "bodies_per_sea" in last(), bad
    assert _raw_set(eng, [members[0], seh.members(64)[1]]) == E_ARG and "same number of waves" in last()
    assert sample() == E_STATE
    # an ensemble of six at one tile each; then a bad component in member 2: the previous ensemble stays in force
    good = seh.ensemble(11, n, 1)
    eng.set_sea_ensemble(good)
    before = eng.sea_ensemble_sample(_tiled(st[:n]), n, 3, DT).clone()
    bad = seh.members(11)
    bad[2] = SeaSpectrum(bad[2].current)
    bad[2].waves = list(members[2].waves[:10]) + [(float("nan"), 0.1, 0.0, 1.0, 0.0)]
    assert _raw_set(eng, bad) == E_ARG and "member 2" in last() and "non-finite" in last()
    bad[2].waves[10] = (-0.1, 0.1, 0.0, 1.0, 0.0)
    assert _raw_set(eng, bad) == E_ARG and "member 2" in last() and "negative amplitude" in last()
    arr, keep = _c_members(members)
    arr[4].wave = None                                             # a NULL wave with waves > 0
    assert eng._lib.hydro_set_sea_ensemble(eng._h, arr, 6, 64) == E_ARG and "null wave" in last()
    for bad_bps in (0, 63, 96):
        assert _raw_set(eng, members, bodies_per_sea=bad_bps) == E_ARG
    assert _raw_set(eng, members, count=0) == E_ARG and _raw_set(eng, members, count=1025) == E_ARG
    assert _same_bits(eng.sea_ensemble_sample(_tiled(st[:n]), n, 3, DT), before)
    # the three-way exclusion, each message naming the call that clears the other kind; clearing with NULL is always allowed
    spec, sea = members[0], SeaState((0.3, 0.0, 0.0)).add_wave(0.1, 0.2, 0.0, 1.4)
    c_spec, keep_spec = _c_members([spec])
    c_sea = nat.Sea()
    c_sea.current[:] = [0.3, 0.0, 0.0]
    assert eng._lib.hydro_set_sea_spectrum(eng._h, ctypes.byref(c_spec[0])) == E_STATE and "hydro_set_sea_ensemble(h, NULL, 0, 0)" in last()
    assert eng._lib.hydro_set_sea(eng._h, ctypes.byref(c_sea)) == E_STATE and "hydro_set_sea_ensemble(h, NULL, 0, 0)" in last()
    assert _same_bits(eng.sea_ensemble_sample(_tiled(st[:n]), n, 3, DT), before)
    assert eng._lib.hydro_set_sea(eng._h, None) == 0 and eng._lib.hydro_set_sea_spectrum(eng._h, None) == 0       # clearing what is not set
    eng.set_sea_ensemble(None)
    eng.set_sea_spectrum(spec)
    assert _raw_set(eng, members) == E_STATE and "hydro_set_sea_spectrum(h, NULL)" in last()
    assert eng._lib.hydro_set_sea_ensemble(eng._h, None, 0, 0) == 0
    eng.set_sea_spectrum(None)
    eng.set_sea(sea)
    assert _raw_set(eng, members) == E_STATE and "hydro_set_sea(h, NULL)" in last()
    assert sample() == E_STATE
    eng.set_sea(None)
    # n needing more members than count: five members at one tile each do not cover six tiles; at two tiles each three do
    eng.set_sea_ensemble(SeaEnsemble(members[:5], 64))
    assert step() == (E_ARG, -7) and "more members" in last()
    assert step(statistics=None, levels=None) == (E_ARG, -7) and "more members" in last()
    assert sample() == E_ARG and "more members" in last()
    # it comes last: the _stat entry's refusals are reported in front of it
    assert step(channels=(7, 0)) == (E_ARG, -7) and "channel" in last()
    assert step(levels=None) == (E_ARG, -7) and "levels" in last()
    assert step(step0=-1) == (E_ARG, -7) and "step0" in last()
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (out, pvo, e8, p2, record, water))
    # the legal launches next to them: 320 bodies are five tiles; and three members of two tiles cover 321
    e8, p2 = _guarded(Extremes.empty(n), S_E), _guarded(np.zeros((n, 2), np.float32), S_P2)
    assert eng._lib.hydro_statistics_reset(eng._h, n, record.data_ptr(), sx.S_ST, eng._stream(None)) == 0
    inputs = (state, prev, lv, a, c17, m27, net)
    was = [b.cpu().numpy() for b in inputs]
    assert step(n_=320, steps=3, extremes=e8, peaks=p2) == (0, 0) and sample(320) == 0
    eng.set_sea_ensemble(SeaEnsemble(members[:3], 128))
    assert step(steps=3, extremes=e8, peaks=p2) == (0, 0) and sample() == 0
    torch.cuda.synchronize()
    # guard bands round every output and the padding lanes
    got, rest = sx.unguard(record.cpu().numpy().view(np.uint32), n)
    assert (got["n"][:320] == 6).all() and got["n"][320] == 3 and (rest == sx.NAN_BITS).all()
    for buf, fields, stride in ((out, 13, S_OUT), (pvo, 6, S_PVO), (e8, 8, S_E), (p2, 2, S_P2), (water, 4, 4 * 64 + 12)):
        bodies, rest = _unguard(buf, n, fields, stride)
        assert np.isnan(rest).all(), "a sentinel of an output was overwritten"
    assert np.isfinite(_unguard(water, n, 4, 4 * 64 + 12)[0]).all()
    assert all(_untouched(b, w) for b, w in zip(inputs, was))
    eng.close()


# ---- 8. the Python paths --------------------------------------------------------------------------------------------------------------------------
def _buoy_field(n):
    c1 = scenes.scene_c1()
    pr = np.tile(c1.params[:1].astype(np.float32), (n, 1))
    mass = float(pr[0, 10])
    z_eq = 0.5 * float(pr[0, 2]) - mass / (c1.rho * float(pr[0, 0] * pr[0, 1]))
    i = np.arange(n) % 128
    st = np.zeros((n, 13), np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = 37.0 * (i % 16), 41.0 * (i // 16), z_eq, 1.0
    return scenes.Scene("sea ensemble", st, np.zeros((n, 6), np.float32), pr, dt=float(np.float32(1.0 / 60.0)), rho=c1.rho, g=c1.g)


def _moored_sim(sc, sea):
    sim = ClosedLoopSim(sc, implicit_drag=True)
    sim.set_sea(sea)
    mass = float(sc.params[0, 10])
    k0, c0 = MooringSpread.for_body(mass, sc.dt, 3)
    centre = sc.state[:, 0:2].astype(np.float64)
    reach = float(np.hypot(15.0, 20.0 + float(sc.state[0, 2])))
    length, k = np.full((sc.n, 3), reach - 0.2), np.full((sc.n, 3), k0)
    lines = MooringSpread.radial(3, 15.0, 20.0, centre=centre, length=length, stiffness=k, damping=c0)
    sim.set_mooring_spread(lines.anchors, length=length, stiffness=k, damping=c0)
    return sim


def test_sim_resident_equals_eager_and_each_member_is_its_own_spectrum_run(native_built):
    """300 buoys - the same 128 positions per member, the third member's block partial - under three seeds: resident, chunked and eager
    runs agree in state, extremes and statistics; and block m of all three is the run of a sim of its own under member m alone."""
    sc = _buoy_field(300)
    ens = jonswap_ensemble(1.5, 7.0, 25.0, seeds=(3, 4, 5), bodies_per_sea=128, spread="cos2", current=(0.4, 0.0, 0.0), g=sc.g)
    records, finals, extremes = {}, {}, {}
    for name, go in (("eager", lambda s: s.run_eager(20)), ("resident", lambda s: s.run_resident(20)), ("chunks", lambda s: s.run_resident(20, chunk=7))):
        sim = _moored_sim(sc, ens)
        assert sim.sea is ens and sim.engine.ensemble_count == 3
        ext, stat = sim.track_extremes(), sim.track_statistics()
        go(sim)
        records[name], finals[name], extremes[name] = stat.record(), sim.state(), ext.bodies()
        if name == "resident":
            assert (stat.count() == 20).all()
            split = ens.split(ext.tension_max())
            assert split.shape == (3, 128) and np.isnan(split[2, 44:]).all() and np.isfinite(split[2, :44]).all()
            assert ens.mean_of_maxima(ext.tension_max()).shape == (128,)
        sim.close()
    for k in ("resident", "chunks"):
        assert sx.same_record(records["eager"], records[k], nan_equal=False), k
        assert np.array_equal(finals["eager"], finals[k]) and np.array_equal(extremes["eager"], extremes[k])
    for m, member in enumerate(ens.members):
        alone = _moored_sim(sc, member)
        ext, stat = alone.track_extremes(), alone.track_statistics()
        alone.run_resident(20)
        block = slice(128 * m, min(128 * (m + 1), 300))
        assert np.array_equal(alone.state()[block], finals["resident"][block]) and np.array_equal(ext.bodies()[block], extremes["resident"][block]), m
        mine = stat.record()
        assert sx.same_record({k: v[block] for k, v in mine.items()}, {k: v[block] for k, v in records["resident"].items()}, nan_equal=False), m
        if m:
            assert not np.array_equal(alone.state()[0:128], finals["resident"][0:128])                   # (and the members do differ)
        alone.close()
    short = ClosedLoopSim(sc, implicit_drag=True)
    with pytest.raises(ValueError, match="do not cover"):
        short.set_sea(SeaEnsemble(ens.members[:2], 128))
    assert short.sea is None
    short.close()


def test_sim_replays_an_ensemble_of_currents_and_refuses_components(native_built):
    sc = _buoy_field(300)
    currents = SeaEnsemble([SeaSpectrum((0.4, -0.1, 0.0)), SeaSpectrum((-0.2, 0.3, 0.0)), SeaSpectrum((0.0, 0.0, 0.0))], 128)
    g, r = _moored_sim(sc, currents), _moored_sim(sc, currents)
    gs, rs = g.track_statistics(("x", "tension")), r.track_statistics(("x", "tension"))
    g.run(64, graph_steps=32)
    r.run_resident(64)
    assert g._graph is not None and sx.same_record(gs.record(), rs.record(), nan_equal=False) and (gs.count() == 64).all()
    assert np.array_equal(g.state(), r.state())
    assert not np.array_equal(g.state()[0:44, 0:2] - sc.state[0:44, 0:2], g.state()[256:300, 0:2] - sc.state[256:300, 0:2])       # the currents differ
    waves = _moored_sim(sc, jonswap_ensemble(1.0, 7.0, 0.0, seeds=range(3), bodies_per_sea=128, g=sc.g))
    with pytest.raises(ValueError, match="graph replays"):
        waves.run(64, graph_steps=32)
    g.clear_sea()
    assert g.sea is None and g.engine.ensemble_count is None
    for s in (g, r, waves):
        s.close()


def test_ensemble_design_loads_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "ensemble_design_loads.py"), "--steps", "240"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    rows = re.findall(r"mean of the maxima +([\d.]+) N +spread over the seeds +([\d.]+) N .*most probable maximum +([\d.]+) N", res.stdout)
    assert len(rows) == 9 and all(float(mean) > 0.0 for mean, _, _ in rows)
    assert "16 seeds x 1152 buoys" in res.stdout
