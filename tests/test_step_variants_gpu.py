"""The instantiations of the fused step kernels that the feature tests do not launch: every family (hydro_step_fused_tiled and
the six hydro_step_fused_tiled_multi* kernels) is dispatched over the flags HALF, NT, IMPLICIT, KE and WARP, and the files that
came with the families launch NT = false and, for the four newer ones, WARP = false only.

1. Non-temporal accesses (hydro_set_tuning(..., non_temporal = 1)) give the bits of temporal ones in every family, over both
   coefficient formats, both drag forms, kinetic energy absent / with / without the rotational term and both semantics; through
   the raw C ABI they keep to their records (guards, strides); and at 131 072 bodies, the smallest size at which the default
   policy streams, the default policy gives the bits of the temporal kernels.
   THE LIMIT OF THIS SECTION: nothing in a launch's outputs says which instantiation produced them.  That non_temporal = 1
   reaches the NT = true kernels rests on streaming_fused() reading the engine's `nt`, which hydro_set_tuning sets; what is
   asserted of the setter is that it refuses a value outside -1, 0, 1.
2. Warp semantics in the applied, pose-hold, sea and bed families: one step against integrator_oracle.integrate of the TRUE
   state with the device's Warp wrench (whose own parity is tests/test_warp_semantics.py's), and the same reference with the
   Numba wrench misses by more than ten bounds.  The populations need no help for that: on the CPU oracle the two semantics'
   wrenches differ by more than 100 x 2^-24 of the wrench scale on 70 .. 98 % of the kept bodies (asserted: at least a quarter),
   so the previous-velocity fields are the designed population's own.
3. The kinetic energy a launch reports with sea, bed, pose hold and applied wrench active is that of the TRUE state it
   returns, not of the sea-relative one; without `rotational` the second element is 0 (include/hydro.h).
4. A body-frame applied wrench in the sea and bed entries: the degenerate equivalences of tests/test_sea_gpu.py and
   tests/test_seabed_gpu.py in that frame, and with an active sea the fp64 step with R a of the true attitude - R^T a misses.

Populations, helpers and references are those of the four feature files; sizes: n = 200 (one block: three full tiles and 8
lanes) and n = 321 (two blocks, the last wave with one live lane); 1 and 7 steps.  One engine per (n, coefficient format) serves
the whole module and is switched with set_tuning / set_semantics / set_sea / set_seabed / set_watch.
Bounds: integrator_oracle.STEP_ULP_BOUND (24) with the surrogate-wrench scales of tests/test_pose_hold_gpu.py and
tests/test_seabed_gpu.py; kinetic energy rel = 1e-12 against scenes.kinetic_energy_fp64; everything else is bit equality
(a NaN equals the NaN with its bits: seven explicit steps may carry a light body out of range).
NO DEVICE FIGURE YET: this file has not run on an MI355X.  With the fp64 oracle rounded to fp32 standing in for the device, the
references of sections 2 and 4 agree within 1 ulp and the wrong ones (Numba wrench, R^T a) miss by more than 5e6; the tests
print the device's figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sea_reference as sr
import seabed_reference as br
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.sea import SeaState
from designed_populations import BED, bed_population, FAR, hold_pop, SEA, SIZES, STEPS  # noqa: F401  (fixtures are requested by name)
from resident_harness import (B, _buffers, COEFFS, DEV, DRAG, DT, _engine, fp64_step_errors, _from, G, _guarded, _k, _ke, _log, NAN, raw, RHO, S_A, S_C, S_IN,
                              S_OUT, S_PV, S_PVO, _same_bits, step_wrench_terms, _tiled, _unguard, _untouched, _watched)

pytestmark = pytest.mark.gpu
FAMILIES = ("single", "multi", "rec", "app", "ctl", "sea", "bed")
SEMANTICS = ("numba", "warp")
KE_MODES = (None, "rotational", "linear")                         # ke_out absent / present with rotational = 1 / with rotational = 0
STEP0 = 7
NT_MIN = 131072                                                   # kNtMinBodies of hydro_kernels.hip
E_ARG = -1


@pytest.fixture(scope="module")
def pops(hold_pop):
    """The first 321 bodies of the designed population three times: as drawn (`hold`), moved by the surface elevation above
    them as in tests/test_sea_gpu.py (`sea`: the partial ones straddle the displaced surface) and sunk onto the bed as in
    tests/test_seabed_gpu.py (`bed`); one set of parameters, applied wrenches and control records for all three."""
    st, pv, params, applied, ctl, _ = hold_pop
    n = max(SIZES)
    sea_st = st[:n].copy()
    sea_st[:, 2] = (sea_st[:, 2].astype(np.float64) + SEA.elevation(sea_st[:, 0], sea_st[:, 1], 0.0)).astype(np.float32)
    bed_st, bed_pv, _ = bed_population(st, pv, params["f32"])
    zero_gains = ctl[:n].copy()
    zero_gains[:, 7:15] = 0.0
    return SimpleNamespace(hold=(st[:n].copy(), pv[:n].copy()), sea=(sea_st, pv[:n].copy()), bed=(bed_st, bed_pv),
                           params={c: params[c][:n].copy() for c in params}, applied=applied[:n].copy(), ctl=ctl[:n].copy(), no_law=zero_gains)


@pytest.fixture(scope="module")
def engines(pops, native_built):
    """engines(n, coeff): the module's one engine of that size and coefficient format, back at its defaults."""
    made = {}

    def get(n, coeff):
        if (n, coeff) not in made:
            made[n, coeff] = _engine(n, pops.params[coeff], coeff)
        eng = made[n, coeff]
        eng.set_tuning()
        eng.set_semantics("numba")
        eng.set_sea(None)
        eng.set_seabed(None)
        eng.set_watch(None)
        return eng
    yield get
    for eng in made.values():
        eng.close()


def _launch(eng, family, cur, old, n, steps, implicit, ke=None, rotational=True, applied=None, control=None, frame="body", log=None,
            wrench=None, step0=STEP0):
    """`steps` steps of one family from (cur, old); returns (the buffer that holds the final state, the other one).  The
    single-step entry is called `steps` times; every other one once."""
    kw = dict(implicit_drag=implicit, ke_out=ke, rotational=rotational)
    rec = dict(log=log, every=1, phase=1, row0=0) if log is not None else {}
    if family == "single":
        for _ in range(steps):
            eng.step_fused_tiled(cur, old, n, DT, wrench=wrench, **kw)
            cur, old = old, cur
        return cur, old
    if family == "multi":
        eng.step_fused_tiled_multi(cur, old, n, DT, steps, **kw)
    elif family == "rec":
        eng.step_fused_tiled_multi_rec(cur, old, n, DT, steps, log, 1, 1, 0, **kw)
    elif family == "app":
        eng.step_fused_tiled_multi_applied(cur, old, n, DT, steps, applied, frame, **rec, **kw)
    elif family == "ctl":
        eng.step_fused_tiled_multi_controlled(cur, old, n, DT, steps, control, applied, frame, **rec, **kw)
    else:
        fn = eng.step_fused_tiled_multi_sea if family == "sea" else eng.step_fused_tiled_multi_bed
        fn(cur, old, n, DT, steps, step0, control, applied, frame, **rec, **kw)
    return old, cur


def _loaded(eng, family, base, n, steps, implicit, ke_mode, watched, a, c17):
    """The loaded form of a family from fresh copies of `base` = (cur, old): (state, other buffer, ke, log, wrench).
    single: with the wrench out.  multi: plain.  rec: the 19-field log.  app: body frame, log.  ctl: control, body-frame applied,
    log.  sea and bed: the same through the sea / over the bed the engine holds."""
    cur, old = base[0].clone(), base[1].clone()
    ke = _ke() if ke_mode else None
    log = _log(steps, len(watched)) if family not in ("single", "multi") else None
    wrench = torch.full((eng.tiles(n), 6, 64), NAN, dtype=torch.float32, device=DEV) if family == "single" else None
    state, other = _launch(eng, family, cur, old, n, steps, implicit, ke, ke_mode != "linear", a if family not in ("single", "multi", "rec") else None,
                           c17 if family in ("ctl", "sea", "bed") else None, "body", log, wrench)
    return state, other, ke, log, wrench


def _assert_same(got, want, what):
    for name, g, w in zip(("state", "prev_out (and the rest of its buffer)", "kinetic energy", "log", "wrench"), got, want):
        assert (g is None) == (w is None), what
        assert g is None or _same_bits(g, w), (name,) + what


# ---- 1. non-temporal = temporal, bit for bit ---------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_non_temporal_gives_the_temporal_bits_in_every_family(coeff, implicit, pops, engines):
    """set_tuning(0, 0, 0) against set_tuning(0, 0, 1), each launch from fresh copies of the same buffers: state out, prev_out
    (with the untouched rest of the buffer it lies in), the kinetic-energy pair, every log row and the single-step entry's
    wrench buffer, NaNs compared as bits."""
    launches = 0
    for n in SIZES:
        eng = engines(n, coeff)
        watched = _watched(n)
        eng.set_watch(watched)
        eng.set_sea(SEA)
        eng.set_seabed(BED)
        a, c17 = _tiled(pops.applied[:n]), _tiled(pops.ctl[:n])
        bases = {which: _buffers(*getattr(pops, which), n) for which in ("sea", "bed")}
        for semantics in SEMANTICS:
            eng.set_semantics(semantics)
            for family in FAMILIES:
                base = bases["bed" if family == "bed" else "sea"]
                for steps in STEPS:
                    for ke_mode in KE_MODES:
                        eng.set_tuning(0, 0, 0)
                        want = _loaded(eng, family, base, n, steps, implicit, ke_mode, watched, a, c17)
                        eng.set_tuning(0, 0, 1)
                        got = _loaded(eng, family, base, n, steps, implicit, ke_mode, watched, a, c17)
                        torch.cuda.synchronize()
                        what = (n, semantics, family, steps, ke_mode)
                        _assert_same(got, want, what)
                        launches += 2
                        # and the comparison is not one of untouched buffers: the launch wrote a state, a log row, an energy
                        state = _from(got[0], n)
                        assert not np.array_equal(state.view(np.uint32), _from(base[0], n).view(np.uint32)), what
                        if steps == 1:
                            assert np.isfinite(state).mean() > 0.9, what
                            assert got[3] is None or not torch.isnan(got[3]).any(), what
                            assert got[2] is None or (torch.isfinite(got[2]).all() and got[2][0] > 0), what
                            assert got[4] is None or np.isfinite(_from(got[4], n)).mean() > 0.9, what
                        assert family == "single" or _same_bits(got[1][:, :7], base[0][:, :7]), what      # the rest of the buffer prev_out lies in
    assert launches == 2 * len(SIZES) * len(SEMANTICS) * len(FAMILIES) * len(STEPS) * len(KE_MODES)


def test_set_tuning_refuses_a_non_temporal_of_two(pops, engines):
    eng = engines(200, "f32")
    assert eng._lib.hydro_set_tuning(eng._h, 0, 0, 2, -1) == E_ARG
    assert eng._lib.hydro_set_tuning(eng._h, 0, 0, -2, -1) == E_ARG
    for ok in (-1, 0, 1):
        assert eng._lib.hydro_set_tuning(eng._h, 0, 0, ok, -1) == 0


@COEFFS
@DRAG
def test_non_temporal_bed_launch_keeps_to_its_records(coeff, implicit, pops, engines):
    """The bed family's loaded launch under non_temporal = 1 through the raw C ABI, n = 200, tile strides larger than F * 64 and
    different for every buffer, NaN in the stride padding and past body n: no sentinel of state_out, prev_out or log is
    overwritten, no input changes, every output is finite and the bodies are those of the tightly packed TEMPORAL launch.
    Three steps with implicit drag, one with explicit drag: explicit steps square the rates of the light bodies here (largest
    |omega| in the fp64 restatement: 1.3e6 rad/s after one step, 2.6e12 after two, 2.6e25 after three - where the squared norm
    of q + dt/2 omega q leaves the fp32 range and the kernel's quaternion is NaN), and a NaN of the model's own would hide one
    read from a sentinel."""
    st, pv = pops.bed
    n, tiles, steps = 200, 4, 3 if implicit else 1
    eng = engines(n, coeff)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch([0, 199])
    state, prev, a, c17 = _guarded(st[:n], S_IN), _guarded(pv[:n], S_PV), _guarded(pops.applied[:n], S_A), _guarded(pops.ctl[:n], S_C)
    before = [b.cpu().numpy() for b in (state, prev, a, c17)]
    out = torch.full((tiles * S_OUT,), NAN, device=DEV)
    pvo = torch.full((tiles * S_PVO,), NAN, device=DEV)
    log = torch.full((4, 19, 8), NAN, device=DEV)
    eng.set_tuning(0, 0, 1)
    rc, written = raw(eng, "bed", n, state, prev, out, pvo, steps=steps, step0=11, implicit=implicit, log=log, fields=19, frame=1, applied=a, control=c17)
    eng._check(rc)
    torch.cuda.synchronize()
    assert written == steps
    got, rest = _unguard(out, n, 13, S_OUT)
    pv_out, prest = _unguard(pvo, n, 6, S_PVO)
    assert np.isnan(rest).all() and np.isnan(prest).all(), "a sentinel of an output was overwritten"
    assert torch.isnan(log[steps:]).all() and torch.isnan(log[:, :, 2:]).all()
    assert all(_untouched(b, was) for b, was in zip((state, prev, a, c17), before))
    assert np.isfinite(got).all() and np.isfinite(pv_out).all(), "a sentinel was read"
    eng.set_tuning(0, 0, 0)
    cur, old = _buffers(st, pv, n)
    want_log = torch.full((4, 19, 8), NAN, device=DEV)
    want, other = _launch(eng, "bed", cur, old, n, steps, implicit, applied=_tiled(pops.applied[:n]), control=_tiled(pops.ctl[:n]), frame="body",
                          log=want_log, step0=11)
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint32), _from(want, n).view(np.uint32))
    assert np.array_equal(pv_out.view(np.uint32), _from(other[:, 7:13], n).view(np.uint32))
    assert _same_bits(log, want_log)
    assert np.array_equal(log[steps - 1, :13, :2].cpu().numpy().T.view(np.uint32), got[[0, 199]].view(np.uint32))     # the last row is the final state


def test_the_default_policy_streams_at_131072_bodies_with_the_temporal_bits(pops, native_built):
    """n = kNtMinBodies: the smallest launch for which non_temporal = -1 picks the streaming kernels.  The 321-body bed
    population tiled to that size; per family one loaded launch of 3 steps, fp16 coefficients, implicit drag, with ke_out, under
    the default tuning and under set_tuning(0, 0, 0)."""
    n, coeff, steps = NT_MIN, "f16", 3
    reps = -(-n // max(SIZES))
    st, pv, pr, applied, ctl = (np.tile(x, (reps, 1))[:n] for x in (*pops.bed, pops.params[coeff], pops.applied, pops.ctl))
    eng = _engine(n, pr, coeff)
    watched = _watched(n)
    eng.set_watch(watched)
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    a, c17, base = _tiled(applied), _tiled(ctl), _buffers(st, pv, n)
    for family in FAMILIES:
        eng.set_tuning(0, 0, 0)
        want = _loaded(eng, family, base, n, steps, True, "rotational", watched, a, c17)
        eng.set_tuning()
        got = _loaded(eng, family, base, n, steps, True, "rotational", watched, a, c17)
        torch.cuda.synchronize()
        _assert_same(got, want, (family,))
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all() and got[2][0] > 0, family
    eng.close()


# ---- 2. Warp semantics against fp64 -------------------------------------------------------------------------------------------------
def _to_world(st, a):
    """R a of the TRUE attitude in fp64, force and torque (as tests/test_applied_wrench_gpu.py builds it)."""
    R = ho._rot_batch(st[:, 3:7].astype(np.float64))
    a64 = a.astype(np.float64)
    return np.concatenate([np.einsum("nab,nb->na", R, a64[:, 0:3]), np.einsum("nab,nb->na", R, a64[:, 3:6])], axis=1)


def _to_world_transposed(st, a):
    R = ho._rot_batch(st[:, 3:7].astype(np.float64))
    a64 = a.astype(np.float64)
    return np.concatenate([np.einsum("nba,nb->na", R, a64[:, 0:3]), np.einsum("nba,nb->na", R, a64[:, 3:6])], axis=1)


def _relative(eng, st, pv, n, step, sea):
    """(s_rel, pv_rel): built on the host in fp32 from hydro_sea_sample's output; without a sea the state itself."""
    if not sea:
        return st[:n], pv[:n]
    w = _from(eng.sea_sample(_tiled(st[:n]), n, step, DT), n)
    return sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])


def _bed_terms(st, pr, bed):
    if not bed:
        return np.zeros((len(st), 6)), np.zeros((len(st), 6))
    touch = br.touching_fp32(BED, st, pr)
    return br.wrench(BED, st, pr, touch), br.wrench_scales(BED, st, pr, touch)


def _device_wrench(eng, s_rel, pv_rel, n):
    return _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)


CASES = {"app-world": ("app", "world"), "app-body": ("app", "body"), "ctl": ("ctl", "body"), "sea": ("sea", "body"), "bed": ("bed", "body")}


@COEFFS
@DRAG
@pytest.mark.parametrize("case", list(CASES))
def test_warp_semantics_one_step_against_fp64(case, coeff, implicit, pops, engines):
    """n = 321, one step, HYDRO_SEM_WARP.  Reference: integrator_oracle.integrate of the TRUE state with (the device's Warp
    wrench of the true state - app, ctl - or of the host-built relative state - sea, bed) + applied (R a in the body frame) +
    the pose-hold law + the fp64 bed wrench with the kernel's own corner decisions; implicit: drag_jacobian of the Warp
    oracle's components.  Bodies within 1e-4 of a branch of the model (in the relative state) are left out.  The same
    reference with the wrench of the SAME engine under Numba semantics must miss by more than ten bounds."""
    family, frame = CASES[case]
    sea, bed = family in ("sea", "bed"), family == "bed"
    n = max(SIZES)
    st, pv = pops.bed if bed else pops.sea if sea else pops.hold
    pr = pops.params[coeff]
    eng = engines(n, coeff)
    eng.set_sea(SEA if sea else None)
    eng.set_seabed(BED if bed else None)
    s_rel, pv_rel = _relative(eng, st, pv, n, STEP0, sea)
    keep = scenes.branch_margins(s_rel, pr) >= 1e-4
    assert keep.mean() > 0.8, keep.mean()
    eng.set_semantics("numba")
    numba = _device_wrench(eng, s_rel, pv_rel, n)
    eng.set_semantics("warp")
    warp = _device_wrench(eng, s_rel, pv_rel, n)
    cur, old = _buffers(st, pv, n)
    got, _ = _launch(eng, family, cur, old, n, 1, implicit, applied=_tiled(pops.applied), control=None if family == "app" else _tiled(pops.ctl), frame=frame)
    torch.cuda.synchronize()
    got = _from(got, n)
    a = _to_world(st, pops.applied) if frame == "body" else pops.applied.astype(np.float64)
    ctl = pops.no_law if family == "app" else pops.ctl             # zero gains: the law's wrench and term magnitudes are zero
    bed_w, bed_s = _bed_terms(st, pr, bed)
    f, t, comps = ho.step_wrench(s_rel, pv_rel, pr, RHO, G, DT, "warp")
    # can the comparison tell the semantics apart?  On the CPU oracle, in units of 2^-24 of the surrogate wrench the bound is measured with
    f_nb, t_nb, _ = ho.step_wrench(s_rel, pv_rel, pr, RHO, G, DT, "numba")
    _, surrogate = step_wrench_terms(st, np.concatenate([f, t], axis=1), applied=a, ctl=ctl, bed_wrench=bed_w, bed_scale=bed_s)
    apart = np.maximum((np.abs(f - f_nb) / (io.ULP * surrogate[:, 0:3])).max(axis=1), np.linalg.norm(t - t_nb, axis=1) / (io.ULP * surrogate[:, 3]))
    assert (apart[keep] > 100.0).mean() >= 0.25, (apart[keep] > 100.0).mean()
    k = None
    if implicit:
        k = _k(comps, s_rel, pr, coeff, n)
        k = (k[0][keep], k[1][keep])
    worst = fp64_step_errors(got[keep], st[keep], warp[keep], pr[keep], k, applied=a[keep], ctl=ctl[keep], bed_wrench=bed_w[keep], bed_scale=bed_s[keep])
    wrong = max(fp64_step_errors(got[keep], st[keep], numba[keep], pr[keep], k, applied=a[keep], ctl=ctl[keep], bed_wrench=bed_w[keep], bed_scale=bed_s[keep]).values())
    print(f"[warp {case} {'implicit' if implicit else 'explicit'} {coeff}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in worst.items())
          + f"  (bound {B:g}); with the Numba wrench: {wrong:.0f}; oracle wrenches apart on {(apart[keep] > 100.0).mean():.0%} of {int(keep.sum())} bodies")
    assert max(worst.values()) <= B, worst
    assert wrong > 10 * B, wrong


# ---- 3. the kinetic energy of the true state ---------------------------------------------------------------------------------------
@COEFFS
@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("family", ["bed", "sea", "ctl"])
def test_kinetic_energy_is_that_of_the_returned_true_state(family, semantics, coeff, pops, engines):
    """Implicit drag.  bed: sea + bed + pose hold + body-frame applied wrench; sea: the sea alone; ctl: the pose hold alone.
    After 1 and 7 steps every returned state is finite and ke_out is scenes.kinetic_energy_fp64 of it to 1e-12; with
    rotational = 0 the second element is 0 ("0 unless `rotational`", include/hydro.h) and the first the same sum.  With a sea:
    the energy of the sea-RELATIVE final state (v - u of hydro_sea_sample at the step the launch ended on) is more than 1e-6
    of the device's away - the comparison would see a kernel that sampled before SeaView::restore."""
    sea, bed = family in ("bed", "sea"), family == "bed"
    st, pv = pops.bed if bed else pops.sea if sea else pops.hold
    pr = pops.params[coeff]
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_semantics(semantics)
        eng.set_sea(SEA if sea else None)
        eng.set_seabed(BED if bed else None)
        a = _tiled(pops.applied[:n]) if bed else None
        c17 = _tiled(pops.ctl[:n]) if family != "sea" else None
        for steps in STEPS:
            for rotational in (True, False):
                cur, old = _buffers(st, pv, n)
                ke = _ke()
                out, _ = _launch(eng, family, cur, old, n, steps, True, ke, rotational, a, c17, "body")
                torch.cuda.synchronize()
                state, pair = _from(out, n), ke.cpu().tolist()
                what = (n, steps, rotational)
                assert np.isfinite(state).all(), what
                lin, rot = scenes.kinetic_energy_fp64(state, pr[:n], rotational=True)
                assert lin > 0 and rot > 0
                assert pair[0] == pytest.approx(lin, rel=1e-12), what
                if rotational:
                    assert pair[1] == pytest.approx(rot, rel=1e-12), what
                else:
                    assert pair[1] == 0.0, what
                if sea:
                    w = _from(eng.sea_sample(out, n, STEP0 + steps, DT), n)
                    relative = state.copy()
                    relative[:, 7:10] = state[:, 7:10] - w[:, 1:4]
                    lin_rel, _ = scenes.kinetic_energy_fp64(relative, pr[:n])
                    assert abs(lin_rel - pair[0]) > 1e-6 * pair[0], (what, lin_rel, pair[0])


# ---- 4. a body-frame applied wrench in the sea and bed entries ---------------------------------------------------------------------
def _all_outputs(eng, family, st, pv, n, steps, implicit, a, c17, watched):
    cur, old = _buffers(st, pv, n)
    ke, log = _ke(), _log(steps, len(watched))
    state, other = _launch(eng, family, cur, old, n, steps, implicit, ke, True, a, c17, "body", log, step0=3)
    return state, other, ke, log, None


@COEFFS
@DRAG
def test_body_frame_without_a_sea_is_the_pose_hold_entry_and_without_a_bed_the_sea_entry(coeff, implicit, pops, engines):
    """frame = "body", the applied wrench with the control record and alone.  No sea and a sea that does not move: the sea entry
    has the bits of hydro_step_fused_tiled_multi_ctl.  No bed and a bed nobody reaches, without a sea and in waves: the bed
    entry has the bits of the sea entry.  State, prev_out, kinetic energy and the 19-field log."""
    st, pv = pops.sea
    still = SeaState()
    for n in SIZES:
        eng = engines(n, coeff)
        watched = _watched(n)
        eng.set_watch(watched)
        a, c17 = _tiled(pops.applied[:n]), _tiled(pops.ctl[:n])
        combos = [(steps, control) for steps in STEPS for control in (c17, None)]
        held = [_all_outputs(eng, "ctl", st, pv, n, steps, implicit, a, control, watched) for steps, control in combos]
        for sea in (None, still, SEA):
            eng.set_sea(sea)
            eng.set_seabed(None)
            through = [_all_outputs(eng, "sea", st, pv, n, steps, implicit, a, control, watched) for steps, control in combos]
            torch.cuda.synchronize()
            for (steps, control), got, want in zip(combos, through, held):
                what = (n, steps, control is None, "moving" if sea is SEA else "no sea" if sea is None else "still")
                if sea is not SEA:
                    _assert_same(got, want, ("sea entry",) + what)
                else:
                    assert not _same_bits(got[0], want[0]), what            # (and the waves do act)
            for bed in (None, FAR):
                eng.set_seabed(bed)
                for (steps, control), want in zip(combos, through):
                    got = _all_outputs(eng, "bed", st, pv, n, steps, implicit, a, control, watched)
                    torch.cuda.synchronize()
                    _assert_same(got, want, ("bed entry", n, steps, control is None, sea is None, bed is None))


@COEFFS
@DRAG
@pytest.mark.parametrize("with_control", [False, True], ids=["applied", "hold+applied"])
def test_body_frame_applied_wrench_in_waves_against_fp64(coeff, implicit, with_control, pops, engines):
    """SEA active, Numba semantics, one step of the sea entry with a body-frame applied wrench.  Reference: the device's wrench
    of the host-built relative state + R a of the TRUE attitude (+ the law), through integrator_oracle.integrate of the true
    state.  The same reference with R^T a must miss by more than ten bounds."""
    st, pv = pops.sea
    pr = pops.params[coeff]
    ctl = pops.ctl if with_control else pops.no_law
    worst, wrong = {}, {}
    for n in SIZES:
        eng = engines(n, coeff)
        eng.set_sea(SEA)
        s_rel, pv_rel = _relative(eng, st, pv, n, STEP0, True)
        keep = scenes.branch_margins(s_rel, pr[:n]) >= 1e-4
        assert keep.mean() > 0.8, (n, keep.mean())
        hydro = _device_wrench(eng, s_rel, pv_rel, n)
        cur, old = _buffers(st, pv, n)
        got, _ = _launch(eng, "sea", cur, old, n, 1, implicit, applied=_tiled(pops.applied[:n]), control=_tiled(pops.ctl[:n]) if with_control else None,
                         frame="body")
        torch.cuda.synchronize()
        got = _from(got, n)
        k = None
        if implicit:
            k = _k(ho.step_wrench(s_rel, pv_rel, pr[:n], RHO, G, DT)[2], s_rel, pr, coeff, n)
            k = (k[0][keep], k[1][keep])
        none = np.zeros((int(keep.sum()), 6))
        for turn, into in ((_to_world, worst), (_to_world_transposed, wrong)):
            a = turn(st[:n], pops.applied[:n])
            into[n] = fp64_step_errors(got[keep], st[:n][keep], hydro[keep], pr[:n][keep], k, applied=a[keep], ctl=ctl[:n][keep], bed_wrench=none, bed_scale=none)
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    missed = {n: max(w.values()) for n, w in wrong.items()}
    print(f"[sea + body-frame applied{' + pose hold' if with_control else ''} {'implicit' if implicit else 'explicit'} {coeff}] max ulps "
          + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items()) + f"  (bound {B:g}); with R^T a: {min(missed.values()):.0f}")
    assert max(per_group.values()) <= B, worst
    assert min(missed.values()) > 10 * B, missed
