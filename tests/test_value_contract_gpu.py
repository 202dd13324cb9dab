"""The value rules of include/hydro.h on the device: tables and checkers are tests/value_contract.py's (shown on the host by
tests/test_value_contract.py), the launches are made here, through the callers of tests/value_contract_launches.py (the population
and engines fixtures, one caller per open-loop entry, `_isolated`, `_everything`), which tests/test_parameter_contract_gpu.py shares.

1. A NON-FINITE BODY IS ITS OWN PROBLEM.  The poison table's bodies - NaN, +-Inf, a zero quaternion, a velocity whose square
   overflows - go through every entry: step_wrench in both previous-velocity modes, step_wrench_tiled plain and _ke, the batch (one
   poisoned scene of three), step_wrench_aos in both quaternion orders, the two _sea open-loop entries, step_components and
   step_components_aos, integrate_tiled, step_fused_tiled, and the resident ladder through `peak` with sea, bed, pose hold, a
   body-frame applied wrench, mooring, extremes, a four-layer net with peaks, the recorder on every body and ke_out - and through
   the rungs above it: `spread` (a spread of three layers), `irr` (a spectrum of 64 components) and `stat` in both its kernel
   families, whose statistics words are one more per-body output.  Every other
   body's outputs have the bits of the launch on the clean population, and a clean launch on the same engine afterwards gives the
   clean bits again.  The same for poisoned rows of the control record; the f_max rows' own step is held to pose_hold_reference
   under STEP_ULP_BOUND.
2. THE EXTREMES FOLD.  The poisoned population with the exact-zero bodies, from a record seeded with NaNs of both signs (one
   with a payload), -0, +0 and a huge value: the record has the bits of Extremes.fold of the launch's own rows (fields = 19) and of
   the per-step tensions (seven one-step launches from the empty record, whose states are the launch's), over 7 steps at once and
   as 3 + 4.  A current and the lines act.  The poison table's bodies leave NaN samples and a speed2 of +Inf, but no infinite
   position: the submerged volume is formed from z, and z = +-Inf gives NaN.  The +-Inf samples are designed like the zeros: two
   dry bodies at x = +Inf and y = -Inf in a sea without waves (no pose hold: 0 x Inf is NaN), and a line with k = +Inf for a
   tension sample of +Inf.  assert_rows_cover asserts that the rows hold every one of these and the +-0 ties: nothing is hoped for.
   hydro_extremes_reset from the poisoned state writes the bits of extremes.seed_of.
3. MALFORMED MOORING, TETHER AND NET RECORDS.  The probes hydro_mooring_wrench and hydro_tether_wrench (with its tension output,
   layer by layer of the net) meet check_probe's (a) .. (e); one step and seven steps of moor, ext, teth, net and peak: a lane that
   adds nothing gives the bits of the launch with its k = c = 0 - in the state, in the wrench the recorder logs, in the extremes
   and peak records -, every well-formed lane has the clean launch's bits after one step, seven steps are seven single steps, and
   the peak record is link_tension_reference.fold of the probe's per-step tensions, a +Inf sample included; the same launches in
   the energy-sampling (ke_out) and streaming (set_tuning(0, 0, 1)) instantiations, where the lanes past n are masked and not
   retired, give the same bits - the dead partner and the lane that names itself among them.

WHY NO VALUE IN A STATE OR A RECORD CAN FORM AN ADDRESS OR A LOOP BOUND (read in silver2_isaacsim_amd/csrc before the first run).
Every load and store of the kernels launched here is addressed by tile (blockIdx and the wave's index), lane (threadIdx & 63),
field (a constant) and a tile stride that the host validated: load_tile_records, store_record, LaneSlots (LDS slots by lane),
the recorder (its column is the watch list's, built on the host from body INDICES), the sea table (indexed by the wave
component j < waves, a host-validated count, read through the constant address space).  The loops run over `steps`, `layers`
and `waves` - host-validated arguments - and over the eight corners of a box; the phase reduction of the sea uses rint of a
float as a VALUE (r = rev - rint(rev)), never as an index.  The data-dependent branches are ballots that skip an evaluation
(bed, mooring, tether): they select code, not addresses.  The one place where a record's value steers data movement is the
tether's partner: `((uint32_t)(int)partner & 63) << 2` is the lane operand of ds_bpermute_b32, which moves registers between
the lanes of ONE wavefront and touches no memory; a lane that is masked off (past n in the last tile - retired by the early return
in the kernels without energy sampling, masked by `if (!KE || live)` in those with it, and retired in the probe) answers +0.  The
peak record's atomic is addressed by tile and lane alone; the bits of T are its operand.  So these tests rely on the header's
"cannot fault" and on this reading; they provoke nothing.  Partners that are not finite or outside the range of int are NOT
tested (the conversion is undefined in C++); the header says what holds for them.

Sizes: n = 200 (three full tiles and 8 live lanes) and n = 321 (two blocks, the last wave with one live lane); 1 and 7 steps; f32
and f16 coefficient records; explicit and implicit drag; both semantics where the harness parametrises them.  One engine per
(n, coefficient format) serves the module.  Bounds: the existing PROBE_BOUND (2) of mooring_reference / tether_reference and
integrator_oracle.STEP_ULP_BOUND; everything else is equality of bits.  The figures of an MI355X are in DESIGN.md section 27."""
import numpy as np
import pytest
import torch

import mooring_reference as mr
import sea_spectrum_reference as ssr
import tether_reference as tr
import value_contract as vc
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd.engine import HydroEngine
from designed_populations import bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import (_buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, fp64_step_errors, _from, _hydro_wrench, _k, NAN, _report, step, _tiled)
from tether_net_population import net_for
from value_contract_launches import (CURRENT, _everything, engines, _isolated, OPEN_LOOP, PER_BODY, pop, SIZES, STEP0, STEPS)  # noqa: F401  (pop, engines: fixtures)

pytestmark = pytest.mark.gpu
FULL = ssr.designed_spectrum()                                    # 64 components
RUNGS = (("spread", None), ("irr", FULL), ("stat", None), ("stat", FULL))


# ---- 1. a non-finite body is its own problem ---------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_a_poisoned_body_is_its_own_problem_in_the_open_loop_entries(coeff, semantics, pop, engines):
    touched = 0
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        st, pv = pop["st"][:n], pop["pv"][:n]
        ps, pp, bodies, names = vc.poison(st, pv, n)
        for name, entry in OPEN_LOOP.items():
            want, got = _isolated(lambda s, p: entry(eng, s, p, n), (st, pv), (ps, pp), bodies, (name, n))
            assert all(np.isfinite(w).all() for w in want), (name, n)
            touched += sum(not vc.same_bits(g[bodies], w[bodies]) for g, w in zip(got, want))
    assert touched >= 2 * len(OPEN_LOOP)                           # (the poison does reach the poisoned bodies' own outputs)


@COEFFS
def test_a_poisoned_scene_of_a_batch_leaves_the_other_scenes_and_its_own_other_bodies(coeff, pop, engines):
    for n in SIZES:
        eng = engines(n, coeff)
        st, pv = pop["st"][:n], pop["pv"][:n]
        ps, pp, bodies, _ = vc.poison(st, pv, n)

        def batch(middle):
            states, prevs = [_tiled(st), _tiled(middle[0]), _tiled(st)], [_tiled(pv), _tiled(middle[1]), _tiled(pv)]
            outs = HydroEngine.step_wrench_tiled_batch([eng] * 3, states, DT, prevs=prevs, ns=[n] * 3)
            return [_from(o, n) for o in outs]
        want, got = batch((st, pv)), batch((ps, pp))
        single = _from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv)), n)
        for k in range(3):
            vc.assert_same_bits(want[k], single, (n, k))
        vc.assert_same_bits(got[0], single, (n, "scene 0"))
        vc.assert_same_bits(got[2], single, (n, "scene 2"))
        vc.assert_isolated(got[1], single, bodies, (n, "the poisoned scene"))
        assert not vc.same_bits(got[1], single)
        for k, w in enumerate(batch((st, pv))):
            vc.assert_same_bits(w, single, (n, k, "afterwards"))


@COEFFS_SEMANTICS
@DRAG
def test_a_poisoned_body_is_its_own_problem_in_the_single_step_entries(coeff, semantics, implicit, pop, engines):
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        st, pv = pop["st"][:n], pop["pv"][:n]
        ps, pp, bodies, _ = vc.poison(st, pv, n)
        wrench = eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv))

        def fused(s, p):
            cur, old = _buffers(s, p, n)
            w = torch.full((eng.tiles(n), 6, 64), NAN, dtype=torch.float32, device=DEV)
            out = eng.step_fused_tiled(cur, old, n, DT, wrench=w, implicit_drag=implicit)
            return [_from(out, n), _from(w, n)]
        _isolated(fused, (st, pv), (ps, pp), bodies, ("step_fused_tiled", n))
        if not implicit:
            _isolated(lambda s, p: [_from(eng.integrate_tiled(_tiled(s), wrench, n, DT), n)], (st, pv), (ps, pp), bodies, ("integrate_tiled", n))


@COEFFS_SEMANTICS
@DRAG
def test_a_poisoned_body_or_control_row_is_its_own_problem_in_the_resident_ladder(coeff, semantics, implicit, pop, engines):
    """`peak` with everything on and ke_out given: the poison table in the state, then in the control record with the state clean.
    Then the same through `spread`, through `irr` under the 64-component spectrum, and through `stat` under the regular sea (the
    _stat kernel family) and under the spectrum (the _irr_stat family)."""
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        st, pv, ctl = pop["st"][:n], pop["pv"][:n], pop["ctl"][:n]
        ps, pp, bodies, _ = vc.poison(st, pv, n)
        bad_ctl, _, _ = vc.poison_control(ctl, st, n)
        net = vc.untie(net_for(pop["net"], n), bodies)
        vc.assert_untied(net, bodies)
        for steps in STEPS:
            run = lambda s, p, c: _everything(eng, pop, n, steps, implicit, st=s, pv=p, ctl=c, net=net, ke=True)  # noqa: E731
            want = run(st, pv, ctl)
            assert (want["peaks"] > 0).sum() >= n // 8 and (want["extremes"][:, 7] > 0).sum() >= n // 8
            for what, got in (("state", run(ps, pp, ctl)), ("control", run(st, pv, bad_ctl))):
                again = run(st, pv, ctl)
                for key in PER_BODY:
                    vc.assert_isolated(got[key], want[key], bodies, (what, key, n, steps))
                    vc.assert_same_bits(again[key], want[key], (what, key, n, steps, "the clean launch afterwards"))
                assert not vc.same_bits(got["state"][bodies], want["state"][bodies])
        # the rungs above `peak`, each kernel family once: the same assertions, with the spread of three layers, the 64-component
        # spectrum and the statistics record (whose eleven words per body are one more per-body output)
        for entry, spectrum in RUNGS:
            for steps in STEPS:
                run = lambda s, p, c: _everything(eng, pop, n, steps, implicit, st=s, pv=p, ctl=c, net=net, ke=True, entry=entry, spectrum=spectrum)  # noqa: E731
                want = run(st, pv, ctl)
                assert (want["peaks"] > 0).sum() >= n // 8 and (want["extremes"][:, 7] > 0).sum() >= n // 8
                assert want["statistics"].shape == (n, 11 if entry == "stat" else 0)
                for what, got in (("state", run(ps, pp, ctl)), ("control", run(st, pv, bad_ctl))):
                    again = run(st, pv, ctl)
                    for key in PER_BODY:
                        vc.assert_isolated(got[key], want[key], bodies, (entry, spectrum is not None, what, key, n, steps))
                        vc.assert_same_bits(again[key], want[key], (entry, spectrum is not None, what, key, n, steps, "the clean launch afterwards"))
                    assert not vc.same_bits(got["state"][bodies], want["state"][bodies])
                    if entry == "stat":                            # the poisoned bodies' records count the steps like everybody's, and differ
                        assert (vc.bits(got["statistics"])[:, 10] == steps).all()
                        assert not vc.same_bits(got["statistics"][bodies], want["statistics"][bodies])


@COEFFS
@DRAG
def test_the_f_max_rows_follow_the_headers_comparison(coeff, implicit, pop, engines):
    """f_max = NaN, 0 and negative on the poison table's bodies, one step of the pose-hold entry against pose_hold_reference (which
    compares as the header does: tests/test_value_contract.py) under STEP_ULP_BOUND; a NaN f_max gives the bits of f_max = +Inf."""
    st, pv, comps = pop["hold"]
    pr = pop["params"][coeff]
    worst = {}
    for n in SIZES:
        eng = engines(n, coeff)
        ctl, bodies, names = vc.poison_control(pop["ctl"], st, n, only=vc.F_MAX_ROWS)
        cur, old = _buffers(st, pv, n)
        hydro = _from(_hydro_wrench(eng, cur, old, n), n)
        got, _ = step(eng, "ctl", cur, old, n, 1, control=_tiled(ctl), implicit=implicit)
        torch.cuda.synchronize()
        got = _from(got, n)
        k = _k(comps(coeff), st, pr, coeff, n) if implicit else None
        worst[n] = fp64_step_errors(got, st[:n], hydro, pr[:n], k, ctl=ctl)
        unlimited = ctl.copy()
        unlimited[np.isnan(unlimited[:, 15]), 15] = np.inf
        cur, old = _buffers(st, pv, n)
        want, _ = step(eng, "ctl", cur, old, n, 1, control=_tiled(unlimited), implicit=implicit)
        vc.assert_same_bits(got, _from(want, n), ("f_max NaN against +Inf", n))
        assert names.count("f_max_nan") >= 3 and names.count("f_max_zero") >= 3 and names.count("f_max_negative") >= 3
    _report(f"pose hold, f_max NaN / 0 / negative, {'implicit' if implicit else 'explicit'} {coeff}", worst)


# ---- 2. the extremes fold, on the device ---------------------------------------------------------------------------------------------------
@COEFFS
@DRAG
def test_the_extremes_record_is_the_fold_of_the_launchs_own_rows(coeff, implicit, pop, engines):
    z = pop["zero"]
    for n in SIZES:
        eng = engines(n, coeff)
        ps, pp, bodies, _ = vc.poison(z["st"], z["pv"], n)
        seed = vc.seeded_record(n)
        run = lambda steps, **kw: _everything(eng, pop, n, steps, implicit, st=ps, pv=pp, ctl=None, moor=z["moor"], net=None, entry="ext", applied=False, bed=None, sea=CURRENT, **kw)  # noqa: E731
        chain = run(7, chunks=[1] * 7)
        whole = run(7, seed=seed)
        vc.assert_same_bits(whole["rows"], chain["rows"], (n, "seven steps are seven single steps"))
        vc.assert_same_bits(whole["state"], chain["state"], n)
        T = _single_step_tensions(eng, pop, n, implicit, ps, pp, z)
        counts = vc.assert_rows_cover(whole["rows"], T, seed)
        print(f"[extremes fold, n = {n}, {coeff}, {'implicit' if implicit else 'explicit'}] samples: {counts}")
        vc.check_extremes(whole["extremes"], whole["rows"], T, seed, (n, "7"))
        split = run(7, seed=seed, chunks=[3, 4])
        vc.assert_same_bits(split["rows"], whole["rows"], (n, "3 + 4 rows"))
        vc.check_extremes(split["extremes"], whole["rows"], T, seed, (n, "3 + 4"))
        assert (T[0] > 0).sum() >= n // 5 and np.isnan(whole["extremes"]).sum() >= 16    # (a quarter of the lines pull in the first step: mooring_population)
        # hydro_extremes_reset from the poisoned state
        record = eng.extremes_reset(torch.full((eng.tiles(n), 8, 64), NAN, dtype=torch.float32, device=DEV), n, _tiled(ps))
        torch.cuda.synchronize()
        vc.assert_same_bits(_from(record, n), ex.seed_of(ps), (n, "reset from a poisoned state"))
        assert np.isnan(ex.seed_of(ps)).any() and np.isinf(ex.seed_of(ps)).any()


def _single_step_tensions(eng, pop, n, implicit, st, pv, z):
    """(7, n) the tension sample of each of seven steps: tension_max of a one-step launch from the EMPTY record, on the chain of
    single steps (+0 where the line adds nothing; a sample is never a NaN: it is T only where T > 0)."""
    eng.set_sea(CURRENT)
    eng.set_seabed(None)
    eng.set_watch(None)
    cur, old = _buffers(st, pv, n)
    lines = _tiled(z["moor"][:n])
    out = []
    for k in range(7):
        record = _tiled(ex.Extremes.empty(n))
        step(eng, "ext", cur, old, n, 1, step0=STEP0 + k, extremes=record, mooring=lines, implicit=implicit)
        cur, old = old, cur
        torch.cuda.synchronize()
        out.append(_from(record, n)[:, 7])
    return np.stack(out)


# ---- 3. malformed mooring, tether and net records -------------------------------------------------------------------------------------------
def _tables(pop, n):
    return (vc.malformed_tethers(pop["rec"], pop["st"], pop["groups"]["pull"], n), vc.malformed_lines(pop["moor"], pop["st"], pop["pulling"], n))


def _with_layer0(net, rec):
    out = np.array(net, np.float32)
    out[:, 0:7] = rec
    return out


def _tether_probe(eng, cur, rec, n):
    T = eng.alloc_tiled(1, n)
    W = eng.tether_wrench(cur, _tiled(rec), n, tension=T)
    return _from(W, n), _from(T, n)[:, 0]


@COEFFS
def test_the_probes_on_malformed_records(coeff, pop, engines):
    totals = {"tether": dict(worst=0.0, pulls=0, nothing=0, non_finite=0), "mooring": dict(worst=0.0, pulls=0, nothing=0, non_finite=0)}
    for n in SIZES:
        eng = engines(n, coeff)
        st = pop["st"][:n]
        cur = _tiled(st)
        teth, moor = _tables(pop, n)
        W, T = _tether_probe(eng, cur, teth.bad, n)
        clean_W, clean_T = _tether_probe(eng, cur, teth.clean, n)
        figures = {"tether": vc.check_probe(teth, st, W, T, clean_W, clean_T, tr.PROBE_BOUND)}
        assert np.isposinf(T[teth.lanes]).sum() == 2 and (clean_T > 0).sum() >= n // 4
        # per layer of the net: layer 0 is the malformed record, the layers behind it are untouched by it
        net = net_for(pop["net"], n)
        bad_net = _with_layer0(net, teth.bad)
        Ws, Ts = eng.tether_net_wrench(cur, _tiled(bad_net), n, 4)
        clean_Ws, clean_Ts = eng.tether_net_wrench(cur, _tiled(net), n, 4)
        vc.assert_same_bits(_from(Ws[0], n), W, (n, "layer 0"))
        vc.assert_same_bits(_from(Ts[0], n)[:, 0], T, (n, "layer 0 tension"))
        for l in (1, 2, 3):
            vc.assert_same_bits(_from(Ws[l], n), _from(clean_Ws[l], n), (n, l))
            vc.assert_same_bits(_from(Ts[l], n), _from(clean_Ts[l], n), (n, l, "tension"))
        # the malformed record in layer 1 behind the clean layer 0: the probe of that layer meets the same checks
        behind = np.concatenate([net[:, 0:7], teth.bad], axis=1)
        Ws, Ts = eng.tether_net_wrench(cur, _tiled(behind), n, 2)
        vc.assert_same_bits(_from(Ws[1], n), W, (n, "as layer 1"))
        vc.assert_same_bits(_from(Ts[1], n)[:, 0], T, (n, "as layer 1, tension"))
        # the mooring line
        W = _from(eng.mooring_wrench(cur, _tiled(moor.bad), n), n)
        clean_W = _from(eng.mooring_wrench(cur, _tiled(moor.clean), n), n)
        figures["mooring"] = vc.check_probe(moor, st, W, None, clean_W, None, mr.PROBE_BOUND)
        for family, f in figures.items():
            totals[family]["worst"] = max(totals[family]["worst"], f["worst"])
            for key in ("pulls", "nothing", "non_finite"):
                totals[family][key] += f[key]
    for family, t in totals.items():
        print(f"[malformed records, {family} probe, {coeff}] worst error {t['worst']:.3f} units of 2^-24 of the scale (PROBE_BOUND "
              f"{(tr if family == 'tether' else mr).PROBE_BOUND:g}); case lanes over n = 200 and 321: {t['pulls']} pull, {t['nothing']} add nothing, "
              f"{t['non_finite']} non-finite")


def _step_cases(pop, n):
    """entry -> (the keyword the malformed record goes by, the table, the record of a launch as a function of the table's record)."""
    teth, moor = _tables(pop, n)
    net = net_for(pop["net"], n)
    return {"moor": ("moor", moor, lambda r: r), "ext": ("moor", moor, lambda r: r), "teth": ("net", teth, lambda r: _with_layer0(net, r)),
            "net": ("net", teth, lambda r: _with_layer0(net, r)), "peak": ("net", teth, lambda r: _with_layer0(net, r))}


def _same_launch(got, want, what, rows=None):
    for key in PER_BODY:
        if key in want:
            g, w = (got[key], want[key]) if rows is None else (got[key][rows], want[key][rows])
            vc.assert_same_bits(g, w, what + (key,))


@COEFFS_SEMANTICS
@DRAG
def test_steps_with_malformed_records(coeff, semantics, implicit, pop, engines):
    minus_zero = 0
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        st, pv, ctl = pop["st"][:n], pop["pv"][:n], pop["ctl"][:n]
        for entry, (key, table, record) in _step_cases(pop, n).items():
            run = lambda rec, steps, **kw: _everything(eng, pop, n, steps, implicit, st=st, pv=pv, ctl=ctl, entry=entry,  # noqa: E731
                                                       **{"net": net_for(pop["net"], n), key: record(rec)}, **kw)
            bad1, bad7 = run(table.bad, 1), run(table.bad, 7)
            # (b) a lane that adds nothing: the bits of the launch with that lane's k = c = 0 - state, logged wrench, records
            _same_launch(bad1, run(vc.neutralised(table, table.kind == "nothing"), 1), (entry, n, 1, "k = c = 0"))
            _same_launch(bad7, run(vc.neutralised(table, table.structural), 7), (entry, n, 7, "k = c = 0"))
            # (e) after one step every well-formed lane has the clean record's bits
            _same_launch(bad1, run(table.clean, 1), (entry, n, 1, "clean"), rows=~table.lanes)
            # seven steps are seven single steps
            chain = run(table.bad, 7, chunks=[1] * 7)
            _same_launch(bad7, chain, (entry, n, 7, "7 x 1"))
            idle = table.lanes & (table.kind == "nothing")
            logged = bad1["rows"][0][idle, 13:19]
            minus_zero += int((np.signbit(logged) & (logged == 0)).sum())
            if entry == "peak":                                    # (f) the fold of the probe's per-step tensions
                net_t = _tiled(record(table.bad))
                starts = [st] + [chain["rows"][k][:, :13] for k in range(6)]                           # the states the seven steps start from
                samples = []
                for s in starts:
                    _, Ts = eng.tether_net_wrench(_tiled(s), net_t, n, 4)
                    samples.append(np.stack([_from(t, n)[:, 0] for t in Ts]))
                samples = np.stack(samples)
                assert np.isposinf(samples).any() and np.isposinf(samples[0, 0]).sum() == 2, (n, "no +Inf sample")
                vc.check_peaks(bad7["peaks"], samples, (n, "peaks of 7 steps"))
                vc.check_peaks(bad1["peaks"], samples[:1], (n, "peaks of 1 step"))
                assert np.isposinf(bad7["peaks"]).sum() >= 2
    print(f"[malformed records in steps, {coeff} {semantics} {'implicit' if implicit else 'explicit'}] components of -0 in the logged wrench "
          f"of the lanes that add nothing: {minus_zero}")


@COEFFS
@DRAG
def test_the_dead_partner_and_the_self_partner_in_the_energy_and_streaming_instantiations(coeff, implicit, pop, engines):
    """`peak` with the malformed net, with ke_out given (the lanes past n are masked, not retired), with set_tuning(0, 0, 1), and with
    both: the bits of the plain launch - which test_steps_with_malformed_records holds to the probe."""
    for n in SIZES:
        eng = engines(n, coeff)
        st, pv, ctl = pop["st"][:n], pop["pv"][:n], pop["ctl"][:n]
        teth, _ = _tables(pop, n)
        case = dict(teth.cases)
        assert teth.kind[case[vc.DEAD]] == "pulls" and teth.kind[case["partner_self"]] == "nothing" and tr.partner(teth.bad)[case[vc.DEAD]] >= n
        net = _with_layer0(net_for(pop["net"], n), teth.bad)
        for steps in STEPS:
            run = lambda **kw: _everything(eng, pop, n, steps, implicit, st=st, pv=pv, ctl=ctl, net=net, **kw)  # noqa: E731
            plain = run()
            _same_launch(run(ke=True), plain, (n, steps, "ke_out"))
            eng.set_tuning(0, 0, 1)
            streamed, both = run(), run(ke=True)
            eng.set_tuning(0, 0, 0)
            _same_launch(streamed, plain, (n, steps, "streaming"))
            _same_launch(both, plain, (n, steps, "streaming, ke_out"))
            dead = case[vc.DEAD]
            assert plain["peaks"][dead, 0] > 0 and plain["rows"][0][dead, 13:16].any()                # the dead partner's pull is in the log
