"""The sheared current on the device (hydro_set_current_profile, hydro_current_profile_sample, hydro_step_fused_tiled_multi_shear).

Everything here is equality of bits, except the one implicit step against fp64:
1. NO PROFILE: the _shear launch is the _fd launch - each option alone, and everything on, in state, prev_out, the log, the extremes,
   the link tensions, every word of the statistics record and the energy pair.
2. CURRENT-ONLY MEMBERS: with waves = 0, U = +0 and a one-knot profile V (no component -0), u = +0 + V = V exactly, so the _shear
   launch is the _fd launch under members whose U is V.
3. THE SAMPLE: u = fl32(u_fd + P), u_fd and eta from hydro_sea_finite_depth_sample and P from the exact restatement of
   tests/current_profile_reference.py at zc formed from that eta - at K = 1, 2, 3, 16 knots under 0, 11 and 64 components, over the
   population the bound was derived on, at steps 0, 7 and 10^6.  The restatement without the last knot must NOT pass.
4. THE COMPOSITION: at 64 components and 16 knots an explicit step equals hydro_step_wrench_tiled on the relative state built from
   hydro_current_profile_sample, then hydro_integrate_tiled on the true state.
5. One implicit step of the same construction against fp64 under integrator_oracle.STEP_ULP_BOUND.
6. 7 steps = 7 x 1 = (2, 5), from step 0 and from 10^6.    7. A body of member m takes the step it takes under member m alone.
8. Every refusal launches nothing and writes nothing; the previous profile stays in force after a refused set.
9. The three runners of ClosedLoopSim, and examples/sheared_current_cable.py.

Shapes: n = 65, 200 and 321; f32 and f16; explicit and implicit drag; both semantics."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import current_profile_reference as cpr
import sea_depth_reference as sdr
import sea_ensemble_harness as seh
import statistics_reference as sx
from conftest import REPO
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.extremes import Extremes
from silver2_isaacsim_amd.sea import CurrentProfile, SeaEnsemble, SeaSpectrum, jonswap
from designed_populations import BED, bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import (B, _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _in_one_allocation, _k, _ke, NAN, RHO, S_A,
                              S_C, S_IN, S_OUT, S_PV, S_PVO, _same_bits, _tiled, _unguard, _untouched, _watched)
from sea_reference import relative
from test_sea_depth_gpu import _fd, _water
from test_sea_ensemble_gpu import (_buoy_field, _equal, _everything, _expected, _levels_for, _moored_sim, pop, _record, _same_or_nan,  # noqa: F401
                                   S_E, S_P2, S_SP3, S_T2)
from tether_net_population import net_for

pytestmark = pytest.mark.gpu
SIZES = (65, 200, 321)
H = cpr.DEPTH
E_ARG, E_STATE = -1, -5
S_W = 4 * 64 + 12
PROFILE = cpr.turning_profile(16)


@pytest.fixture(scope="module", autouse=True)
def _return_the_cached_blocks():
    """As tests/test_sea_depth_gpu.py: this module leaves no blocks behind in torch's caching allocator."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _sea(waves, n, tps=1):
    """The harness's ensemble for n bodies at the depth H."""
    return _fd(seh.ensemble(waves, n, tps), H)


# ---- 1. no profile ----------------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_without_a_profile_the_launch_is_the_fd_launch_with_everything_on(coeff, implicit, pop, native_built):
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_seabed(BED)
        _water(eng, _sea(11, n))
        for was_set in (False, True):
            if was_set:                                            # a profile that was set and cleared again is no profile
                eng.set_current_profile(PROFILE)
                eng.set_current_profile(None)
            for bare in (False, True):
                want = _everything(eng, "fd", pop, n, 7, 5, implicit, bare=bare, ke=_ke())
                got = _everything(eng, "shear", pop, n, 7, 5, implicit, bare=bare, ke=_ke())
                assert set(got) == set(want) and _equal(got, want, n) is None, (n, bare, _equal(got, want, n))
                assert _same_bits(got["ke"], want["ke"])
                want = _everything(eng, "fd", pop, n, 1, 5, implicit, bare=bare, record=False)
                got = _everything(eng, "shear", pop, n, 1, 5, implicit, bare=bare, record=False)
                assert set(got) == set(want) and all(_same_or_nan(got[k], want[k]) for k in got), (n, bare)
        eng.close()


@COEFFS_SEMANTICS
def test_without_a_profile_the_launch_is_the_fd_entrys_with_each_option_alone(coeff, semantics, pop, native_built):
    """n = 65, 2 steps, with the kinetic energy - each option alone, and none, with and without a record, in still water, in a
    regular sea, under a spectrum, under an ensemble and in a finite-depth sea."""
    n, steps, step0 = 65, 2, 3
    st, pv = pop["st"], pop["pv"]
    lev = _tiled(_levels_for(st, n))
    spec = seh.members(11)[2]
    from designed_populations import SEA
    for option in (None, "log", "applied", "control", "sea", "spectrum", "ensemble", "depth", "seabed", "spread", "extremes", "net", "peaks"):
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        eng.set_watch([0, 5, 63, 64])
        _water(eng, SEA if option == "sea" else spec if option == "spectrum" else seh.ensemble(11, n, 1) if option == "ensemble"
               else _sea(11, n) if option == "depth" else None)
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
            want, got = run("fd", with_record), run("shear", with_record)
            assert len(got) == len(want) and all(_same_bits(x, y) for x, y in zip(got, want)), (option, with_record)
        eng.close()


def test_every_existing_entry_ignores_a_profile(pop, native_built):
    """With a profile set, the _fd entry and the _fd sample give the bits they give without one; the _shear entry does see it."""
    n = 200
    eng = _engine(n, pop["params"]["f32"], "f32")
    _water(eng, _sea(11, n))
    want = _everything(eng, "fd", pop, n, 2, 5, False, bare=True)
    sample = eng.sea_finite_depth_sample(_tiled(pop["st"][:n]), n, 5, DT).clone()
    eng.set_current_profile(PROFILE)
    assert _equal(_everything(eng, "fd", pop, n, 2, 5, False, bare=True), want, n) is None
    assert _same_bits(eng.sea_finite_depth_sample(_tiled(pop["st"][:n]), n, 5, DT), sample)
    moved = _everything(eng, "shear", pop, n, 2, 5, False, bare=True)
    fraction, every_tile = sdr.differs(_from(moved["state"], n), _from(want["state"], n), n)
    assert fraction >= 0.75 and every_tile, (fraction, every_tile)
    assert not _same_bits(eng.current_profile_sample(_tiled(pop["st"][:n]), n, 5, DT), sample)
    eng.set_current_profile(None)
    assert _same_bits(eng.current_profile_sample(_tiled(pop["st"][:n]), n, 5, DT), sample)          # without a profile: the _fd sample's bits
    eng.close()


# ---- 2. current-only members ------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_a_one_knot_profile_over_still_members_is_the_fd_launch_under_that_current(coeff, implicit, pop, native_built):
    v = (0.4, -0.3, 0.05)
    for n in SIZES:
        tiles = (n + 63) // 64
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_seabed(BED)
        for bare in (False, True):
            _water(eng, SeaEnsemble([SeaSpectrum(v, H) for _ in range(tiles)], 64))
            want = _everything(eng, "fd", pop, n, 7, 5, implicit, bare=bare, ke=_ke())
            _water(eng, SeaEnsemble([SeaSpectrum((0.0, 0.0, 0.0), H) for _ in range(tiles)], 64))
            still = _everything(eng, "fd", pop, n, 7, 5, implicit, bare=bare, ke=_ke())
            assert _equal(still, want, n) is not None                     # (the current moves the bodies)
            eng.set_current_profile(CurrentProfile([-0.5 * H], [v]))
            got = _everything(eng, "shear", pop, n, 7, 5, implicit, bare=bare, ke=_ke())
            eng.set_current_profile(None)
            assert set(got) == set(want) and _equal(got, want, n) is None, (n, bare, _equal(got, want, n))
            assert _same_bits(got["ke"], want["ke"])
        eng.close()


# ---- 3. the sample ----------------------------------------------------------------------------------------------------------------------------
def _seas():
    full = sdr.designed_sea()
    return {0: SeaSpectrum(full.current, H), 11: sdr.truncated(full, 11), 64: full}


def test_sample_is_the_fd_sample_plus_the_exact_restatement_bit_for_bit(pop, native_built):
    seas = _seas()
    eng = _engine(256, pop["params"]["f32"], "f32")
    told_apart = 0
    for knots in cpr.KNOTS:
        prof = cpr.turning_profile(knots)
        st = cpr.population(prof, extra=90)
        n = len(st)
        assert 64 < n <= 256
        state = _tiled(st)
        for count, sea in seas.items():
            _water(eng, sea, n)
            eng.set_current_profile(prof)
            for step in (0, 7, 10 ** 6):
                fd = _from(eng.sea_finite_depth_sample(state, n, step, DT), n)
                got = _from(eng.current_profile_sample(state, n, step, DT), n)
                zc = cpr.clamped_depth(st[:, 2], fd[:, 0], H)
                want = fd[:, 1:4] + cpr.profile_exact(prof, zc)                      # one fp32 add per component
                assert want.dtype == np.float32 and np.array_equal(got[:, 0].view(np.uint32), fd[:, 0].view(np.uint32)), (knots, count, step)
                assert np.array_equal(got[:, 1:4].view(np.uint32), want.view(np.uint32)), (knots, count, step)
                short = fd[:, 1:4] + (cpr.profile_exact(prof, zc, drop_last=True) if knots > 1 else np.float32(0.0))
                assert not np.array_equal(got[:, 1:4].view(np.uint32), short.view(np.uint32)), (knots, count, step)
                told_apart += 1
                # and the restatement itself stands within the bound of the fp64 profile
                assert cpr.profile_errors(prof, zc, cpr.profile_exact(prof, zc)) <= cpr.PROFILE_BOUND
    assert told_apart == 4 * 3 * 3
    eng.close()


# ---- 4. the composition -----------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_explicit_step_is_wrench_of_the_relative_state_then_integrator_of_the_true_one(coeff, semantics, pop, native_built):
    st, pv = pop["st"], pop["pv"]
    for n in SIZES:
        eng = _engine(n, pop["params"][coeff], coeff, semantics)
        watched = _watched(n, (0, 63, 64))
        eng.set_watch(watched)
        ens = _sea(64, n)
        assert len(ens.members[0].waves) == 64 and PROFILE.knots == 16
        _water(eng, ens)
        eng.set_current_profile(PROFILE)
        for step0 in (0, 7):
            w = _from(eng.current_profile_sample(_tiled(st[:n]), n, step0, DT), n)
            s_rel, pv_rel = relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
            wrench = eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel))
            cur, old = _buffers(st, pv, n)
            want = eng.integrate_tiled(cur, wrench, n, DT)
            log = torch.full((1, 19, len(watched)), NAN, dtype=torch.float32, device=DEV)
            got, got_prev = seh.launch(eng, cur, old, n, 1, step0=step0, entry="shear", log=log, every=1, phase=1, row0=0)
            cur, old = _buffers(st, pv, n)
            plain, _ = seh.launch(eng, cur, old, n, 1, step0=step0, entry="fd")
            torch.cuda.synchronize()
            fraction, every_tile = sdr.differs(_from(want, n), _from(plain, n), n)       # the condition: the profile moves nearly every body
            assert fraction >= 0.75 and every_tile, (n, fraction, every_tile)
            assert _same_bits(got, want), (n, step0)
            assert np.array_equal(got_prev.cpu().numpy().view(np.uint32), scenes.to_tiled(st[:n, 7:13]).view(np.uint32))    # the TRUE velocity
            host = log.cpu().numpy()[0]
            assert np.array_equal(host[:13].T.view(np.uint32), _from(want, n)[watched].view(np.uint32)), (n, step0)
            assert np.array_equal(host[13:].T.view(np.uint32), _from(wrench, n)[watched].view(np.uint32)), (n, step0)
        eng.close()


# ---- 5. one implicit step against fp64 ----------------------------------------------------------------------------------------------------------
@COEFFS
def test_implicit_step_against_fp64(coeff, pop, native_built):
    """tests/test_sea_spectrum_gpu.py's construction: the relative state formed on the host from hydro_current_profile_sample, the
    device's hydrodynamic wrench of it, the drag coefficients of integrator_oracle.drag_jacobian on the relative state, and
    integrator_oracle.integrate of the TRUE state; left out, as there: bodies within 1e-4 of a branch of the hydrodynamic model."""
    st, pv, pr = pop["st"], pop["pv"], pop["params"][coeff]
    worst = {}
    for n in SIZES:
        eng = _engine(n, pr, coeff)
        _water(eng, _sea(64, n))
        eng.set_current_profile(PROFILE)
        w = _from(eng.current_profile_sample(_tiled(st[:n]), n, 7, DT), n)
        s_rel, pv_rel = relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.5, (n, keep.mean())
        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
        cur, old = _buffers(st, pv, n)
        got, _ = seh.launch(eng, cur, old, n, 1, step0=7, entry="shear", implicit=True)
        torch.cuda.synchronize()
        got = _from(got, n)
        k = _k(ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2], s_rel, pr, coeff, n)
        worst[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], (k[0][keep], k[1][keep]))
        eng.close()
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[one implicit step, 64 components, 16 knots, {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items())
          + f"  (bound {B:g}); worst {max(per_group.values()):.2f}")
    assert max(per_group.values()) <= B, worst


# ---- 6. chunking ------------------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_one_launch_equals_single_steps_and_chunks(coeff, implicit, pop, native_built):
    n = 321
    eng = _engine(n, pop["params"][coeff], coeff)
    eng.set_seabed(BED)
    eng.set_current_profile(PROFILE)
    for tps in (1, 2):
        _water(eng, _sea(64, n, tps))
        for step0 in (0, 10 ** 6):
            whole = _everything(eng, "shear", pop, n, 7, step0, implicit)
            for chunks in ([1] * 7, [2, 5]):
                parts = _everything(eng, "shear", pop, n, 7, step0, implicit, chunks=chunks)
                assert _equal(parts, whole, n) is None, (tps, step0, chunks, _equal(parts, whole, n))
            assert (stx.unpack(whole["record"].cpu().numpy(), n)["n"] == 7).all()
    eng.close()


# ---- 7. members -------------------------------------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_every_block_takes_the_step_it_takes_under_its_member_alone(coeff, implicit, pop, native_built):
    for n, tps in ((200, 1), (321, 2)):
        eng = _engine(n, pop["params"][coeff], coeff)
        eng.set_seabed(BED)
        eng.set_current_profile(PROFILE)
        ens = _sea(11, n, tps)
        for bare in (False, True):
            runs = []
            for m in ens.members:                                  # member m alone, over everybody
                _water(eng, m, n)
                runs.append(_everything(eng, "shear", pop, n, 3, 5, implicit, bare=bare))
            _water(eng, ens)
            got = _everything(eng, "shear", pop, n, 3, 5, implicit, bare=bare)
            want = _expected(runs, n, tps)
            assert _equal(got, want, n) is None, (n, tps, bare, _equal(got, want, n))
        eng.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def _raw_set(eng, knots, z, v):
    zf = (ctypes.c_float * max(len(z), 1))(*z) if z is not None else None
    vf = (ctypes.c_float * max(len(v), 1))(*v) if v is not None else None
    c = nat.CurrentProfile(knots, ctypes.cast(zf, ctypes.POINTER(ctypes.c_float)) if zf is not None else None,
                           ctypes.cast(vf, ctypes.POINTER(ctypes.c_float)) if vf is not None else None)
    return eng._lib.hydro_set_current_profile(eng._h, ctypes.byref(c))


def test_refusals_launch_nothing_write_nothing_and_keep_the_previous_profile(pop, native_built):
    n = 321
    tiles = (n + 63) // 64
    eng = _engine(n, pop["params"]["f32"], "f32")
    last = lambda: eng._lib.hydro_last_error(eng._h).decode()  # noqa: E731
    st, pv = pop["st"], pop["pv"]
    lev = _levels_for(st, n)
    state, prev, lv = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(lev, sx.S_LV)
    a, c17 = _guarded(pop["applied"][:n], S_A), _guarded(pop["ctl"][:n], S_C)
    m27, net = _guarded(pop["spread"][:n, 0:27], S_SP3), _guarded(net_for(pop["net"], n, 2), S_T2)
    fresh = lambda stride: torch.full((tiles * stride,), NAN, device=DEV)  # noqa: E731
    e8, p2, out, pvo, record, water = fresh(S_E), fresh(S_P2), fresh(S_OUT), fresh(S_PVO), fresh(sx.S_ST), fresh(S_W)
    # one allocation in a fixed order (resident_harness._in_one_allocation): no call here hands a buffer over as another record, so no
    # claimed extent runs past its buffer - the arena only takes the allocator's placement out of the test, as in tests/test_statistics_gpu.py
    state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record, water = _in_one_allocation(state, prev, lv, a, c17, m27, net, e8, p2, out, pvo, record, water)
    everything = dict(applied=a, s_applied=S_A, control=c17, s_control=S_C, mooring=m27, s_mooring=S_SP3, layers=3, extremes=e8, s_extremes=S_E,
                      tether=net, s_tether=S_T2, net_layers=2, peaks=p2, s_peaks=S_P2, statistics=record, s_statistics=sx.S_ST, levels=lv, s_levels=sx.S_LV)

    def step(n_=n, **kw):
        args = dict(everything)
        args.update(kw)
        return seh.raw_ens(eng, n_, state, prev, out, pvo, entry="shear", **args)

    def sample(n_=n):
        return eng._lib.hydro_current_profile_sample(eng._h, n_, state.data_ptr(), S_IN, 3, DT, water.data_ptr(), S_W, eng._stream(None))
    good_z, good_v = [-9.0, -3.0, 0.0], [0.0, 0.0, 0.0, 0.3, 0.1, 0.0, 0.5, -0.2, 0.02]
    bad_sets = [((-1, good_z, good_v), "knots out of range"), ((17, good_z, good_v), "knots out of range"),
                ((3, None, good_v), "null z or v"), ((3, good_z, None), "null z or v"),
                ((3, [-9.0, float("nan"), 0.0], good_v), "non-finite"), ((3, [-9.0, -float("inf"), 0.0], good_v), "non-finite"),
                ((3, good_z, good_v[:4] + [float("inf")] + good_v[5:]), "non-finite"), ((3, good_z, good_v[:8] + [float("nan")]), "non-finite"),
                ((3, [-9.0, -3.0, 0.5], good_v), "z > 0"), ((3, [-9.0, -9.0, 0.0], good_v), "strictly ascending"),
                ((3, [-3.0, -9.0, 0.0], good_v), "strictly ascending"),
                ((3, [-9.0, -1.5e-45, 0.0], good_v), "out of fp32 range"),                                   # inv = 1 / 1.4e-45
                ((3, good_z, [-3e38, 0.0, 0.0, 3e38, 0.0, 0.0, 0.0, 0.0, 0.0]), "out of fp32 range")]        # D = 6e38
    # the sample without a finite-depth sea, with and without a profile; the setter's refusals with nothing set before: nothing becomes set
    assert sample() == E_STATE and "hydro_set_sea_finite_depth" in last()
    for args, msg in bad_sets:
        assert _raw_set(eng, *args) == E_ARG and msg in last(), (args, last())
    assert step() == (0, 0)                                        # no profile became set: the _fd entry's launch, in still water
    torch.cuda.synchronize()
    out.fill_(NAN), pvo.fill_(NAN), e8.fill_(NAN), p2.fill_(NAN), record.fill_(NAN)
    # a profile set whether or not a sea is set; then the step and the sample without a finite-depth sea: HYDRO_E_STATE, whatever else is set
    assert _raw_set(eng, 3, good_z, good_v) == 0
    for other in (None, seh.members(11)[0], seh.ensemble(11, n, 1)):
        _water(eng, other)
        assert step() == (E_STATE, -7) and "hydro_set_sea_finite_depth" in last() and "current profile" in last(), other
        assert step(statistics=None, levels=None) == (E_STATE, -7) and "hydro_set_sea_finite_depth" in last()
        assert sample() == E_STATE and "hydro_set_sea_finite_depth" in last()
        # it comes last: the _fd entry's refusals are reported in front of it
        assert step(channels=(7, 0)) == (E_ARG, -7) and "channel" in last()
        assert step(levels=None) == (E_ARG, -7) and "levels" in last()
        assert step(step0=-1) == (E_ARG, -7) and "step0" in last()
        assert step(n_=n + 1) == (E_ARG, -7)
    # with a finite-depth sea: every refused set leaves the previous profile in force
    _water(eng, _sea(11, n))
    before = eng.current_profile_sample(_tiled(st[:n]), n, 3, DT).clone()
    assert not _same_bits(before, eng.sea_finite_depth_sample(_tiled(st[:n]), n, 3, DT))
    for args, msg in bad_sets:
        assert _raw_set(eng, *args) == E_ARG and msg in last(), (args, last())
    assert _same_bits(eng.current_profile_sample(_tiled(st[:n]), n, 3, DT), before)
    # n needing more members than count: five members at one tile each do not cover six tiles
    eng.set_sea_finite_depth(SeaEnsemble(_sea(11, n).members[:5], 64))
    assert step() == (E_ARG, -7) and "more members" in last()
    assert sample() == E_ARG and "more members" in last()
    assert step(channels=(7, 0)) == (E_ARG, -7) and "channel" in last()
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (out, pvo, e8, p2, record, water))
    # the legal launches next to them: 320 bodies are five tiles; and three members of two tiles cover 321
    e8, p2 = _guarded(Extremes.empty(n), S_E), _guarded(np.zeros((n, 2), np.float32), S_P2)
    assert eng._lib.hydro_statistics_reset(eng._h, n, record.data_ptr(), sx.S_ST, eng._stream(None)) == 0
    inputs = (state, prev, lv, a, c17, m27, net)
    was = [b.cpu().numpy() for b in inputs]
    assert step(n_=320, steps=3, extremes=e8, peaks=p2) == (0, 0) and sample(320) == 0
    eng.set_sea_finite_depth(SeaEnsemble(_sea(11, n).members[:3], 128))
    assert step(steps=3, extremes=e8, peaks=p2) == (0, 0) and sample() == 0
    torch.cuda.synchronize()
    # guard bands round every output and the padding lanes
    got, rest = sx.unguard(record.cpu().numpy().view(np.uint32), n)
    assert (got["n"][:320] == 6).all() and got["n"][320] == 3 and (rest == sx.NAN_BITS).all()
    for buf, fields, stride in ((out, 13, S_OUT), (pvo, 6, S_PVO), (e8, 8, S_E), (p2, 2, S_P2), (water, 4, S_W)):
        bodies, rest = _unguard(buf, n, fields, stride)
        assert np.isnan(rest).all(), "a sentinel of an output was overwritten"
    assert np.isfinite(_unguard(water, n, 4, S_W)[0]).all()
    assert all(_untouched(b, w) for b, w in zip(inputs, was))
    # clearing: NULL and knots = 0 (the arrays are not looked at)
    assert _raw_set(eng, 0, None, None) == 0 and eng._lib.hydro_set_current_profile(eng._h, None) == 0
    assert _same_bits(eng.current_profile_sample(_tiled(st[:n]), n, 3, DT), eng.sea_finite_depth_sample(_tiled(st[:n]), n, 3, DT))
    eng.close()


# ---- 9. the Python paths ------------------------------------------------------------------------------------------------------------------------
def test_sim_resident_equals_eager_and_the_profile_changes_the_run(native_built):
    """300 moored buoys under a JONSWAP sea built for h = 9 m and a tide plus a wind-driven slab on another heading: resident, chunked
    and eager runs agree in state, extremes and statistics; without the profile the run is another; graph replays and a sea without
    a depth are refused."""
    sc = _buoy_field(300)
    sea = jonswap(1.5, 7.0, 25.0, seed=3, depth=H, spread="cos2", current=(0.1, 0.0, 0.0), g=sc.g)
    prof = CurrentProfile.power_law(0.8, 10.0, H, knots=12) + CurrentProfile.slab(0.3, 100.0, 3.0)
    records, finals, extremes = {}, {}, {}
    for name, go in (("eager", lambda s: s.run_eager(20)), ("resident", lambda s: s.run_resident(20)), ("chunks", lambda s: s.run_resident(20, chunk=7)),
                     ("run", lambda s: s.run(20, graph_steps=0))):
        sim = _moored_sim(sc, sea)
        sim.set_current_profile(prof)
        assert sim.current_profile is prof and sim.engine.current_profile is prof and sim.engine.finite_depth == H
        ext, stat = sim.track_extremes(), sim.track_statistics()
        go(sim)
        records[name], finals[name], extremes[name] = stat.record(), sim.state(), ext.bodies()
        if name == "resident":
            assert (stat.count() == 20).all() and np.isfinite(finals[name]).all()
            with pytest.raises(ValueError, match="graph replays"):
                sim.run(64, graph_steps=32)
            sim.clear_sea()
            with pytest.raises(ValueError, match="needs a water column"):
                sim.run_resident(2)
            sim.clear_current_profile()
            assert sim.current_profile is None and sim.engine.current_profile is None
            sim.run_resident(2)                                    # still water, no profile: legal again
        sim.close()
    for k in ("resident", "chunks", "run"):
        assert sx.same_record(records["eager"], records[k], nan_equal=False), k
        assert np.array_equal(finals["eager"], finals[k]) and np.array_equal(extremes["eager"], extremes[k]), k
    plain = _moored_sim(sc, sea)
    plain.run_resident(20)
    assert not np.array_equal(plain.state(), finals["resident"])
    plain.close()


def test_sheared_current_cable_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "sheared_current_cable.py"), "--steps", "240"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    rows = re.findall(r"ROV offset +([\d.]+) m uniform +([\d.]+) m sheared", res.stdout)
    assert len(rows) == 1 and float(rows[0][1]) < float(rows[0][0])                # the sheared current loads the cable less below the surface
    assert "uniform" in res.stdout and "sheared" in res.stdout
