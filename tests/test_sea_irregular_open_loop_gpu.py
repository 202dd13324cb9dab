"""The spectrum, the ensemble and the finite-depth sea in the open-loop entries on the device (hydro_step_wrench_tiled_irr,
hydro_step_wrench_aos_irr) and in the plugin.

1. THE COMPOSITION (no tolerance): a step is, bit for bit, the parent entry on the relative state built on the host, with fp32
   subtractions, from the kind's own sample at (1, time) - for a lone spectrum, an ensemble and a finite-depth sea at h = 9 m; the
   engine's record receives the TRUE velocity; the rows entry gives the same force and torque bits in either quaternion order.
2. THE LADDER DOWNWARDS (no tolerance): up to 8 components are the _sea entry under the same SeaState; an 8-wave sea, no sea, a
   still spectrum and one of amplitude 0 are the _sea entry and the parents; h = 1e6 m is the deep launch (the two host
   conditions of DESIGN.md section 32 asserted first); a body of member m takes the launch under the lone spectrum m.
3. THE CLOSED LOOP: one explicit step of step_fused_tiled_multi_fd at step0 is _irr(time = step0 * DT), then integrate_tiled.
4. THE FP64 ORACLE on the fp32 relative state, within the project's gate of 1e-5.
5. REFUSALS launch nothing and write nothing; legal launches stay inside their bands.  6. VALUE RULES.  7. REPLAY.  8. PLUGIN.
9. The example.

Population, seas and the condition under which these identities mean something: tests/irregular_open_loop_cases.py; the condition
itself is asserted on the fp64 reference alone in tests/test_sea_irregular_open_loop.py.  No new tolerance is introduced here: the
water's own error is bounded where the samples are (SPECTRUM_VIEW_BOUND, DEPTH_VIEW_BOUND) and reaches these entries through 1."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irregular_open_loop_cases as ic
import sea_depth_reference as sdr
import sea_ensemble_harness as seh
import value_contract as vc
from conftest import REPO
from oracle import hydro_oracle as ho
from silver2_isaacsim_amd import behavior as hb
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.engine import HydroEngine
from silver2_isaacsim_amd.sea import jonswap, SeaEnsemble, SeaSpectrum, SeaState
from silver2_isaacsim_amd.testing import build_main_scene
from designed_populations import hold_pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import (_buffers, COEFFS_SEMANTICS, DEV, DT, _engine, _from, G, _guarded, NAN, RHO, S_IN, S_PV, _same_bits, _tiled, _unguard,
                              _untouched)
from sea_reference import relative

pytestmark = pytest.mark.gpu
S_WR = 6 * 64 + 44                                                # the wrench's tile stride in the guard tests
E_ARG = -1


@pytest.fixture(scope="module")
def pop(hold_pop):
    st, pv, params = ic.near_surface(*hold_pop[:3])
    return {"st": st, "pv": pv, "params": params}


def _water(eng, water, n=None):
    """The engine's water: None, a SeaState, a SeaSpectrum, a SeaEnsemble, or either of the two with a depth - whatever was set
    before is cleared first."""
    eng.set_sea(None)
    eng.set_sea_spectrum(None)
    eng.set_sea_ensemble(None)
    eng.set_sea_finite_depth(None)
    if water is None:
        return
    if getattr(water, "depth", None) is not None:
        eng.set_sea_finite_depth(water, n)
    elif isinstance(water, SeaEnsemble):
        eng.set_sea_ensemble(water)
    elif isinstance(water, SeaSpectrum):
        eng.set_sea_spectrum(water)
    else:
        eng.set_sea(water)


def _rows(st, n, xyzw):
    """The simulator's tensors of bodies 0 .. n - 1: positions, orientations (wxyz, or xyzw), velocities."""
    q = st[:n, 3:7] if xyzw else st[:n, [6, 3, 4, 5]]
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (st[:n, 0:3], q, st[:n, 7:13]))


def _sample(eng, st, n, time):
    """(n, 4) [eta, u]: the existing sample of the kind the engine holds, at (1, time) or (0, .)."""
    step, dt = (1, float(time)) if time > 0.0 else (0, 1.0)
    sample = eng.sea_finite_depth_sample if eng.finite_depth is not None else eng.sea_ensemble_sample if eng.ensemble_count is not None \
        else eng.sea_spectrum_sample
    return _from(sample(_tiled(st[:n]), n, step, dt), n)


def _relative_at(eng, st, pv, n, time):
    w = _sample(eng, st, n, time)
    return relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])


def _prev_is(eng, v6):
    return np.array_equal(eng.get_prev_velocity().cpu().numpy().T.view(np.uint32), np.ascontiguousarray(v6).view(np.uint32))


def _composition(eng, st, pv, n, time, what):
    """Test 1's body for one engine state, one n and one time."""
    true_state, true_prev, true_vel = _tiled(st[:n]), _tiled(pv[:n]), st[:n, 7:13]
    s_rel, pv_rel = _relative_at(eng, st, pv, n, time)
    assert vc.same_bits(_from(eng.irregular_sea_sample_at(true_state, n, time), n), _sample(eng, st, n, time)), what
    rel_state = _tiled(s_rel)
    want = eng.step_wrench_tiled(rel_state, n, DT, prev=_tiled(pv_rel))                 # caller-owned previous velocity
    assert _same_bits(eng.step_wrench_tiled_irr(true_state, n, DT, time, prev=true_prev), want), what
    eng.set_prev_velocity(pv[:n])                                                       # engine-owned: the same wrench, the TRUE velocity kept
    assert _same_bits(eng.step_wrench_tiled_irr(true_state, n, DT, time), want), what
    assert _prev_is(eng, true_vel), what
    want_f, want_t = eng.unpack_wrench_aos(want, n)
    for xyzw in (False, True):
        eng.set_prev_velocity(pv[:n])
        f, t = eng.step_wrench_aos_irr(*_rows(st, n, xyzw), DT, time, quat_xyzw=xyzw)
        assert _same_bits(f, want_f) and _same_bits(t, want_t), (what, xyzw)
        assert _prev_is(eng, true_vel), (what, xyzw)
    return s_rel


# ---- 1. the composition ------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_step_is_the_parent_entry_on_the_relative_state_of_the_kinds_own_sample(coeff, semantics, pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    for k, n in enumerate(ic.SIZES):
        eng = _engine(n, params, coeff, semantics)
        for count in (ic.COUNTS if n == 65 else (ic.COUNTS[k],)):
            for sea in (ic.lone(count), ic.at_depth(ic.lone(count))):
                _water(eng, sea, n)
                for time in ic.TIMES:
                    s_rel = _composition(eng, st, pv, n, time, (n, count, sea.depth, time))
                    assert n == 1 or (s_rel[:, 2] != st[:n, 2]).mean() > 0.9
        if n == 257:                                              # the streaming instantiations (non-temporal loads, write-through stores)
            eng.set_tuning(non_temporal=1)
            for sea in (ic.lone(63), ic.at_depth(ic.lone(63))):
                _water(eng, sea, n)
                _composition(eng, st, pv, n, ic.TIMES[2], (n, "streaming", sea.depth))
        eng.close()


@COEFFS_SEMANTICS
def test_every_block_steps_through_its_own_member(coeff, semantics, pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    for n in sorted({n for n, _ in ic.ENSEMBLE_CASES}):
        eng = _engine(n, params, coeff, semantics)
        for tps in (t for m, t in ic.ENSEMBLE_CASES if m == n):
            for count in (11, 64):
                ens = seh.ensemble(count, n, tps)
                for sea in (ens, ic.at_depth(ens)):
                    _water(eng, sea)
                    for time in (ic.TIMES[0], ic.TIMES[2], ic.TIMES[4]):
                        _composition(eng, st, pv, n, time, (n, tps, count, sea.depth, time))
                    # a body of member m takes the launch under the lone spectrum m (test 2's last rung)
                    time = ic.TIMES[2]
                    whole = _from(eng.step_wrench_tiled_irr(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n])), n)
                    for m, member in enumerate(sea.members):
                        a, b = m * sea.bodies_per_sea, min((m + 1) * sea.bodies_per_sea, n)
                        _water(eng, member, n)
                        alone = _from(eng.step_wrench_tiled_irr(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n])), n)
                        assert vc.same_bits(whole[a:b], alone[a:b]), (n, tps, count, m)
                        if m:
                            assert not vc.same_bits(whole[0:a], alone[0:a])     # (and the members differ)
        eng.close()


# ---- 2. the ladder downwards ---------------------------------------------------------------------------------------------------------------
def _three(eng, entry, st, pv, n, time=None):
    """(tiled wrench with a caller-owned prev, with the engine's own, forces and torques of the rows entry) through `entry`:
    "" the parents, "_sea" or "_irr"."""
    args = () if time is None else (time,)
    tiled, rows = getattr(eng, "step_wrench_tiled" + entry), getattr(eng, "step_wrench_aos" + entry)
    a = tiled(_tiled(st[:n]), n, DT, *args, prev=_tiled(pv[:n])).clone()
    eng.set_prev_velocity(pv[:n])
    b = tiled(_tiled(st[:n]), n, DT, *args).clone()
    eng.set_prev_velocity(pv[:n])
    f, t = (x.clone() for x in rows(*_rows(st, n, False), DT, *args))
    return a, b, f, t


def _same_three(got, want):
    return all(_same_bits(x, y) for x, y in zip(got, want))


@COEFFS_SEMANTICS
def test_up_to_eight_components_are_the_sea_entry_and_degenerate_seas_the_parents(coeff, semantics, pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    full = ic.lone(8)
    for n in (65, 257):
        eng = _engine(n, params, coeff, semantics)
        for k in range(1, 9):
            spectrum, state = sdr.truncated(full, k), SeaState(full.current)
            for w in full.waves[:k]:
                state.add_wave(*w)
            for time in (0.0, 7.0 * DT, 0.123456789):
                _water(eng, state)
                want = _three(eng, "_sea", st, pv, n, time)
                assert _same_three(_three(eng, "_irr", st, pv, n, time), want), (n, k, time)      # an 8-wave sea: exactly the _sea launch
                _water(eng, spectrum)
                assert _same_three(_three(eng, "_irr", st, pv, n, time), want), (n, k, time)
                if k == 8 and time > 0.0:
                    assert _same_three(_three(eng, "_sea", st, pv, n, time), _three(eng, "", st, pv, n))     # _sea ignores a spectrum
        _water(eng, None)
        parents = _three(eng, "", st, pv, n)
        flat = SeaSpectrum()
        for w in full.waves:
            flat.add_wave(0.0, *w[1:])
        for sea in (None, SeaSpectrum(), flat, ic.at_depth(SeaSpectrum()), ic.at_depth(flat), SeaEnsemble([flat] * 5, 64), SeaState()):
            _water(eng, sea, n)
            for time in (0.0, 0.7):
                assert _same_three(_three(eng, "_irr", st, pv, n, time), parents), (n, time)       # sign of zero included
                assert _same_three(_three(eng, "_sea", st, pv, n, time), parents), (n, time)
                assert _prev_is(eng, st[:n, 7:13])
        eng.close()


@COEFFS_SEMANTICS
def test_in_deep_water_the_finite_depth_launch_is_the_deep_launch(coeff, semantics, pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    assert (np.abs(st[:, 2]) < 1000.0).all()
    for count in (11, 64):
        for m in seh.members(count):
            consts, q = sdr.device_constants(m, ic.FAR)
            assert min(math.hypot(w[1], w[2]) for w in m.waves) >= 0.01 and all(x == 0.0 for x in q)
            assert all(float(c[7]) + float(c[3]) * 1000.0 < -200.0 for c in consts)           # gl_j - kl2_j zc for zc >= -1 000 m
    for n, tps in ((65, 1), (321, 1), (321, 2)):
        eng = _engine(n, params, coeff, semantics)
        for count in (11, 64):
            for sea in (ic.lone(count, 3), seh.ensemble(count, n, tps)):
                for time in (0.0, 7.0 * DT, 1e6 * DT):
                    _water(eng, sea, n)
                    want = _three(eng, "_irr", st, pv, n, time)
                    _water(eng, ic.at_depth(sea, ic.FAR), n)
                    assert _same_three(_three(eng, "_irr", st, pv, n, time), want), (n, tps, count, time)
        eng.close()


# ---- 3. the closed loop ----------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_explicit_closed_loop_step_is_this_wrench_then_the_integrator(coeff, semantics, pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    for n, count in ((65, 11), (257, 64)):
        eng = _engine(n, params, coeff, semantics)
        for sea in (ic.lone(count), ic.at_depth(ic.lone(count))):
            _water(eng, sea, n)
            for step0 in (0, 7, 10 ** 6):
                cur, old = _buffers(st, pv, n)
                wrench = eng.step_wrench_tiled_irr(cur, n, DT, float(step0) * DT, prev=old)
                want = eng.integrate_tiled(cur, wrench, n, DT)
                got, _ = seh.launch(eng, cur, old, n, 1, step0=step0, entry="fd")
                torch.cuda.synchronize()
                assert _same_bits(got, want), (n, sea.depth, step0)
        eng.close()


# ---- 4. fp64 -------------------------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_wrench_against_the_fp64_oracle_on_the_relative_state(coeff, semantics, pop, native_built):
    """hydro_oracle.step_wrench on the fp32 relative state the device formed (test 1: the host-built one, bit for bit), error by
    hydro_oracle.wrench_error, gate 1e-5: the parent kernel's arithmetic on those inputs.  Measured on an MI355X: see DESIGN.md
    section 33."""
    st, pv, params = pop["st"], pop["pv"], pop["params"][coeff]
    n, time = ic.N, 7.0 * DT
    eng = _engine(n, params, coeff, semantics)
    worst = {}
    for name, sea in (("spectrum", ic.lone(64)), ("ensemble", seh.ensemble(64, n, 1)), ("h = 9 m", ic.at_depth(seh.ensemble(64, n, 2)))):
        _water(eng, sea, n)
        s_rel, pv_rel = _relative_at(eng, st, pv, n, time)
        got = _from(eng.step_wrench_tiled_irr(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n])), n)
        eng.set_prev_velocity(pv[:n])
        f, t = eng.step_wrench_aos_irr(*_rows(st, n, False), DT, time)
        ref_f, ref_t, _ = ho.step_wrench(s_rel, pv_rel, params[:n], RHO, G, DT, semantics=semantics)
        err = ho.wrench_error(got[:, 0:3], got[:, 3:6], ref_f, ref_t, params[:n], RHO, G)
        err_aos = ho.wrench_error(f.cpu().numpy(), t.cpu().numpy(), ref_f, ref_t, params[:n], RHO, G)
        worst[name] = (float(err.max()), float(err_aos.max()))
    eng.close()
    print(f"[open-loop irregular sea, {coeff} {semantics}] largest wrench_error against fp64 on the relative state (tiled, rows): "
          + "  ".join(f"{k} {a:.3e} {b:.3e}" for k, (a, b) in worst.items()) + f"  (gate {ic.GATE:g})")
    assert max(max(v) for v in worst.values()) <= ic.GATE, worst


# ---- 5. refusals and guards, through the raw C ABI --------------------------------------------------------------------------------------------
def _banded(n, pad=16):
    buf = torch.full((pad + 3 * n + pad,), NAN, device=DEV)
    return buf, buf.data_ptr() + 4 * pad


def _band_rows(buf, n, pad=16):
    host = buf.cpu().numpy()
    return host[pad:pad + 3 * n].reshape(n, 3), np.concatenate([host[:pad], host[pad + 3 * n:]])


def test_refusals_launch_nothing_and_legal_launches_stay_inside(pop, native_built):
    st, pv, params = pop["st"], pop["pv"], pop["params"]["f32"]
    n, tiles = 257, 5
    eng = _engine(n, params, "f32")
    lib, h, stream = eng._lib, eng._h, eng._stream(None)
    last = lambda: lib.hydro_last_error(h)  # noqa: E731
    state, prev = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV)
    before = [b.cpu().numpy() for b in (state, prev)]
    wrench = torch.full((tiles * S_WR,), NAN, device=DEV)
    (fbuf, f_ptr), (tbuf, t_ptr) = _banded(n), _banded(n)
    pos, quat, vel = _rows(st, n, False)
    marker = np.ascontiguousarray(pv[:n][::-1])                   # what the engine's record holds: no refused call may touch it
    eng.set_prev_velocity(marker)

    def tiled(time=1.0, n_=n, s=state.data_ptr(), ss=S_IN, p=prev.data_ptr(), ps=S_PV, dt=DT, w=wrench.data_ptr(), ws=S_WR):
        return lib.hydro_step_wrench_tiled_irr(h, n_, s, ss, p, ps, dt, w, ws, time, stream)

    def aos(time=1.0, n_=n, p=pos.data_ptr(), q=quat.data_ptr(), v=vel.data_ptr(), dt=DT, f=f_ptr, t=t_ptr):
        return lib.hydro_step_wrench_aos_irr(h, n_, p, q, 0, v, dt, f, t, time, stream)

    bad_times = (float("nan"), float("inf"), float("-inf"), -1e-300, -1.0, float(2 ** 52 + 1), 1e300)
    members = seh.members(11)
    short = SeaEnsemble(members[:4], 64)                          # four members at one tile each do not cover five tiles
    for sea in (ic.lone(11), seh.ensemble(11, n, 1), ic.at_depth(seh.ensemble(11, n, 2)), short, ic.at_depth(short), SeaState((0.3, 0.0, 0.0)), None):
        _water(eng, sea, n)                                       # `time` is validated whatever the engine holds
        for time in bad_times:
            assert tiled(time) == E_ARG and b"time must be finite" in last(), time
            assert aos(time) == E_ARG and b"time must be finite" in last(), time
        # the time is looked at first
        assert tiled(-1.0, n_=n + 1) == E_ARG and b"time must be finite" in last()
        assert aos(-1.0, dt=0.0) == E_ARG and b"time must be finite" in last()
        # then the parents' refusals, in front of the members'
        for kw in (dict(n_=n + 1), dict(n_=-1), dict(dt=0.0), dict(dt=float("nan")), dict(s=None), dict(w=None), dict(w=wrench.data_ptr() + 4),
                   dict(ws=6 * 64 - 4), dict(ss=13 * 64 + 2), dict(p=prev.data_ptr() + 8), dict(ps=6 * 64 - 4), dict(ws=1 << 24)):
            assert tiled(**kw) == E_ARG and b"more members" not in last(), kw
        for kw in (dict(n_=n + 1), dict(n_=(1 << 26) + 1), dict(dt=0.0), dict(p=None), dict(f=None), dict(t=None), dict(t=t_ptr + 4), dict(f=f_ptr + 8),
                   dict(v=vel.data_ptr() + 4)):
            assert aos(**kw) == E_ARG and b"more members" not in last(), kw
        if sea is short or getattr(sea, "members", None) is not None and len(sea.members) == 4:
            # too few members: _ens's (_fd's) message and status, last
            which = b"finite-depth sea" if sea.depth is not None else b"sea ensemble"
            assert tiled() == E_ARG and b"n needs more members than the " + which in last()
            assert tiled(p=None, ps=0) == E_ARG and b"more members" in last()          # the engine's own prev: its record is not acquired either
            assert aos() == E_ARG and b"n needs more members than the " + which in last()
            torch.cuda.synchronize()                              # nothing was launched or written, the engine's record included
            assert torch.isnan(wrench).all() and torch.isnan(fbuf).all() and torch.isnan(tbuf).all() and _prev_is(eng, marker)
            assert tiled(n_=256) == 0 and aos(n_=256) == 0                           # four tiles are covered
            torch.cuda.synchronize()
            wrench.fill_(NAN); fbuf.fill_(NAN); tbuf.fill_(NAN)
            eng.set_prev_velocity(marker)
    torch.cuda.synchronize()
    assert torch.isnan(wrench).all() and torch.isnan(fbuf).all() and torch.isnan(tbuf).all()
    assert all(_untouched(b, was) for b, was in zip((state, prev), before)) and _prev_is(eng, marker)

    # the legal launches next to them: the largest time there is, the bodies' fields and nothing else
    for sea in (ic.lone(64), seh.ensemble(11, n, 1), ic.at_depth(seh.ensemble(64, n, 2))):
        _water(eng, sea, n)
        for time in (float(2 ** 52), 0.0, 1.0):
            wrench.fill_(NAN); fbuf.fill_(NAN); tbuf.fill_(NAN)
            assert tiled(time) == 0
            eng.set_prev_velocity(pv[:n])
            assert aos(time) == 0
            torch.cuda.synchronize()
            got, rest = _unguard(wrench, n, 6, S_WR)
            (f, f_band), (t, t_band) = _band_rows(fbuf, n), _band_rows(tbuf, n)
            assert np.isfinite(got).all() and np.isnan(rest).all(), "a sentinel of the tiled wrench was read or overwritten"
            assert np.isfinite(f).all() and np.isfinite(t).all() and np.isnan(f_band).all() and np.isnan(t_band).all()
            assert all(_untouched(b, was) for b, was in zip((state, prev), before)), "a caller-owned prev: nothing is written but the wrench"
            assert _prev_is(eng, st[:n, 7:13])
            want = eng.step_wrench_tiled_irr(_tiled(st[:n]), n, DT, time, prev=_tiled(pv[:n]))
            assert np.array_equal(got.view(np.uint32), _from(want, n).view(np.uint32))
            assert np.array_equal(np.concatenate([f, t], axis=1).view(np.uint32), got.view(np.uint32))
    eng.close()


# ---- 6. value rules ------------------------------------------------------------------------------------------------------------------------------
def test_a_body_at_infinity_or_nan_poisons_nobody(pop, native_built):
    n = ic.N
    eng = _engine(n, pop["params"]["f32"], "f32")
    bodies = vc.poisoned_bodies(n)
    others = np.setdiff1d(np.arange(n), bodies)
    rows = [r for r in vc.POISONS if r[0] in ("nan_z", "+inf_z", "-inf_z")]
    assert len(rows) == 3
    st, pv, time = pop["st"], pop["pv"], 7.0 * DT
    for sea in (ic.lone(64), seh.ensemble(64, n, 1), ic.at_depth(seh.ensemble(64, n, 1))):
        _water(eng, sea, n)
        clean = _three(eng, "_irr", st, pv, n, time)
        clean = (_from(clean[0], n), _from(clean[1], n), clean[2].cpu().numpy(), clean[3].cpu().numpy())
        assert all(np.isfinite(c).all() for c in clean)
        for name, _, cols, value in rows:
            bad = st.copy()
            bad[np.ix_(bodies, cols)] = value
            got = _three(eng, "_irr", bad, pv, n, time)
            got = (_from(got[0], n), _from(got[1], n), got[2].cpu().numpy(), got[3].cpu().numpy())
            for g, c in zip(got, clean):
                vc.assert_same_bits(g[others], c[others], (name, sea.depth))
    eng.close()


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_captured_prepared_rows_step_with_a_spectrum_replays_to_the_eager_bits(pop, native_built):
    st, pv = pop["st"], pop["pv"]
    n = ic.N
    eng = _engine(n, pop["params"]["f16"], "f16")
    eng.set_sea_spectrum(ic.lone(64))
    pos, quat, vel = _rows(st, n, False)
    f = torch.full((n, 3), NAN, device=DEV)
    t = torch.full((n, 3), NAN, device=DEV)
    step = eng.prepare_step_wrench_aos(pos, quat, vel, f, t)
    eng.set_prev_velocity(pv[:n])
    step(DT, None, 2.5)
    torch.cuda.synchronize()
    want_f, want_t = f.clone(), t.clone()
    eng.set_prev_velocity(pv[:n])
    direct_f, direct_t = eng.step_wrench_aos_irr(pos, quat, vel, DT, 2.5)               # the prepared step issued the _irr entry
    assert _same_bits(direct_f, want_f) and _same_bits(direct_t, want_t)
    still_f, _ = (x.clone() for x in eng.step_wrench_aos(pos, quat, vel, DT))
    f.fill_(NAN); t.fill_(NAN)
    stream = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            step(DT, stream, 2.5)
        torch.cuda.synchronize()
        assert torch.isnan(f).all()                               # capturing records, it does not execute
        eng.set_prev_velocity(pv[:n])
        g.replay()
        stream.synchronize()
    assert _same_bits(f, want_f) and _same_bits(t, want_t)
    assert not _same_bits(want_f, still_f)                        # and the sea is in it
    eng.close()


# ---- 8. the plugin ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [None, ic.DEPTH], ids=["spectrum", "depth"])
@pytest.mark.parametrize("batched", [True, "callbacks", False], ids=["scene", "callbacks", "per-prim"])
def test_plugin_applies_the_direct_call_at_its_clock(batched, depth, native_built):
    hb.REGISTRY.clear()
    world, host, prims, behaviors = build_main_scene(batched)
    n = len(prims)
    sea = jonswap(1.2, 7.0, 25.0, seed=5, spread="cos2", current=(0.3, -0.1, 0.0), depth=depth)
    behaviors[0].set_sea(sea)
    for b in behaviors:
        b.on_play()
    rows = np.stack([b._param_row(float(world.masses[i])) for i, b in enumerate(behaviors)])
    direct = HydroEngine(n, DEV, behaviors[0]._rho, behaviors[0]._g)     # the scene scalars as the prims' float attributes hold them
    direct.set_params(rows)
    _water(direct, sea, n)
    dts = (1.0 / 60.0, 0.02, 1.0 / 90.0)
    time = 0.0
    applied = lambda: (torch.stack([world.applied[p.path][0] for p in prims]), torch.stack([world.applied[p.path][1] for p in prims]))  # noqa: E731
    for k, dt in enumerate(dts):
        host.step(dt)
        want_f, want_t = direct.step_wrench_aos_irr(world.positions, world.orientations, world.velocities, dt, time)
        torch.cuda.synchronize()
        got_f, got_t = applied()
        assert _same_bits(got_f, want_f) and _same_bits(got_t, want_t), (k, time)
        if k == 1:
            still_f, _ = direct.step_wrench_aos_sea(world.positions, world.orientations, world.velocities, dt, time)     # _sea ignores this sea
            assert not _same_bits(want_f, still_f)                # (the record it leaves is the same TRUE velocity)
        time = time + dt
        world.velocities += 0.01 * torch.randn_like(world.velocities)          # "PhysX" moves the bodies
        world.positions += 0.01 * torch.randn_like(world.positions)
    assert behaviors[-1].sea_time == (dts[0] + dts[1]) + dts[2]
    # clearing the sea returns to the bits of step_wrench_aos
    behaviors[0].set_sea(None)
    host.step(dts[0])
    want_f, want_t = direct.step_wrench_aos(world.positions, world.orientations, world.velocities, dts[0])
    torch.cuda.synchronize()
    got_f, got_t = applied()
    assert _same_bits(got_f, want_f) and _same_bits(got_t, want_t)
    for b in behaviors:
        b.on_stop()
    direct.close()
    hb.REGISTRY.clear()


# ---- 9. the example --------------------------------------------------------------------------------------------------------------------------------
def test_plugin_buoy_in_irregular_sea_example(native_built):
    res = subprocess.run([sys.executable, os.path.join(REPO, "examples", "plugin_buoy_in_irregular_sea.py"), "--steps", "240"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    print(res.stdout)
    assert "largest |z - z_eq - eta| over 240 steps" in res.stdout and "drift:" in res.stdout and "64 components, deep water" in res.stdout
