"""The parameter record's rule (include/hydro.h "Parameter record") on the device: the table and the checkers
are tests/parameter_cases.py's (shown on the host instantiation by tests/test_parameter_contract.py), the launches are made here
through the callers of tests/value_contract_launches.py.

1. EVERY WRENCH ENTRY.  The table dealt onto the population with the dry bodies (lanes 0, 31, 32, 63, the first and the last live
   lane of the last tile, every third body: at most a third), through step_wrench in both previous-velocity modes,
   step_wrench_tiled plain and _ke, step_wrench_aos in both quaternion orders, the batch (a dealt scene beside a clean one), the
   two _sea entries with a sea set, step_components and _aos; f32 and f16 coefficients, both semantics.  Every other body has the
   bits of the launch with the clean record, the case bodies meet `check_rows`, and the entries agree with each other bit for bit
   on the case bodies too (a NaN equals a NaN).  The _sea entries evaluate the state relative to the water: they meet `check_rows`
   with the rule of that state (built on the host in fp32 from hydro_sea_sample's output, as the kernels subtract), on every case
   body on which the row is decisive under the sea as well, and are equal to each other bit for bit.
2. THE f16 STORAGE.  An f16 engine given the raw table equals, on every output of every entry above and of one fused step, an f32
   engine given the record rounded through numpy's half: ties, subnormals, underflow, -0, NaN and +-Inf of the device conversion.
3. THE REFUSAL.  hydro_set_params_f16 with a finite coefficient of magnitude >= 65520 returns HYDRO_E_ARG, names the field and the
   first body and hydro_set_params_f32, and writes nothing: the step after it has the bits of the step before - host and device
   arrays, through C and through HydroEngine.set_params.
4. THE STEPS.  hydro_integrate_tiled, hydro_step_fused_tiled (explicit and implicit) and the resident ladder's last entry,
   hydro_step_fused_tiled_multi_spread, with everything on - sea, bed, pose hold, applied wrench, a three-layer spread, a two-layer
   net with its link tensions, extremes, every body recorded: isolation bit for bit over 1 and 7 steps and (2, 5) chunks - state,
   prev_out, log, extremes, peaks; one step of the case bodies, fused and in the ladder, against integrator_oracle.integrate with
   the constants as given (`check_step`, STEP_ULP_BOUND).  hydro_seabed_wrench: isolation, and every row of dims and mass against
   the header's fp32 operations restated (an infinite dimension: isolation).
5. KINETIC ENERGY.  Stand-alone and sampled by the tiled wrench and the fused step, one launch per sub-table (the finite rows
   together, each non-finite row alone): scenes.kinetic_energy_fp64 of the constants as given, 1e-12 where finite (a negative mass
   gives a negative energy), not finite where it is not.

WHY NO CONSTANT CAN FAULT (read in silver2_isaacsim_amd/csrc before the first run).  The parameter record is loaded by tile, lane
and a constant field offset (load_tile_records; kPrmTileF32 / kPrmTileF16 times the tile index); no value of it is converted to an
integer, none bounds a loop (steps, layers, waves, the eight corners of a box) and the branches it feeds (the degenerate height, the
bed's and the lines' ballots) select code, not addresses.  The one float-to-int conversion of the kernels is the tether's partner,
which is a tether record's, not a constant.  The range check of hydro_set_params_f16 reads body i < n of the caller's seven
coefficient arrays and adds one atomic minimum on a word of its own.  So these launches provoke nothing."""
import numpy as np
import pytest
import torch

import mooring_reference as mr
import mooring_spread_reference as msr
import parameter_cases as pc
import sea_reference as sr
import seabed_reference as br
import tether_net_reference as tnr
import tether_reference as tr
import value_contract as vc
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.engine import HydroEngine
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import TIES
from mooring_spread_population import spread_population
from resident_harness import _buffers, COEFFS, COEFFS_SEMANTICS, DEV, DRAG, DT, _from, G, _ke, _log, NAN, RHO, _rows, step_wrench_terms, _tiled
from tether_net_population import net_for
from tether_population import bodies_of
from value_contract_launches import engines, OPEN_LOOP, PER_BODY, pop, SIZES, STEP0, TIME  # noqa: F401  (pop, engines: fixtures)

pytestmark = pytest.mark.gpu
WRENCH = ("step_wrench, engine-owned previous velocity", "step_wrench, caller-owned previous velocity", "step_wrench_tiled",
          "step_wrench_tiled_ke", "step_wrench_aos wxyz", "step_wrench_aos xyzw")
SEA_ENTRIES = ("step_wrench_tiled_sea", "step_wrench_aos_sea")
COMPONENTS = ("step_components", "step_components_aos")
assert set(WRENCH + SEA_ENTRIES + COMPONENTS) == set(OPEN_LOOP)


def _flat(outputs):
    """A caller's list of (n, F) arrays as one (n, sum F) array: F | T, or the eight vectors | the ratio."""
    return np.concatenate([np.asarray(o, np.float32) for o in outputs], axis=1)


def _population(pop, n):
    z = pop["zero"]
    st, pv = z["st"][:n], z["pv"][:n]
    return st, pv, pc.suitable(st, pv, pop["params"]["f32"][:n])


def _accel32(st, pv):
    with np.errstate(all="ignore"):
        return ((st[:, 7:13] - pv) / np.float32(DT)).astype(np.float32)


def _used(params, coeff):
    return pc.half_rounded(params) if coeff == "f16" else params


def _cut(rule, idx):
    return tuple(np.asarray(a)[idx] for a in rule[:3])


def _batch(eng, st, pv, n, clean_engine):
    """The dealt scene beside a clean one: (the dealt scene's wrench, the clean scene's)."""
    outs = HydroEngine.step_wrench_tiled_batch([eng, clean_engine], [_tiled(st), _tiled(st)], DT, prevs=[_tiled(pv), _tiled(pv)], ns=[n, n])
    return _from(outs[0], n), _from(outs[1], n)


# ---- 1. every wrench entry ---------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
def test_every_wrench_entry_computes_the_constants_as_given(coeff, semantics, pop, engines):
    checked = deviations = under_sea = 0
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        beside = HydroEngine(n, DEV, RHO, G)                          # the clean scene of the batch
        beside.set_params(pop["params"][coeff][:n], coeff)
        beside.set_semantics(semantics)
        st, pv, (wet, dry, finite) = _population(pop, n)
        a32 = _accel32(st, pv)
        clean_params = pop["params"]["f32"][:n]
        eng.set_sea(SEA)                                               # the state the _sea entries evaluate: relative to the water they sample
        water = _from(eng.sea_sample_at(_tiled(st), n, TIME), n)
        eng.set_sea(None)
        s_rel, pv_rel = sr.relative(st, pv, water[:, 0], water[:, 1:4])
        wet_sea, dry_sea, _ = pc.suitable(np.nan_to_num(s_rel), np.nan_to_num(pv_rel), clean_params)
        try:
            eng.set_params(clean_params, coeff)
            clean = {name: _flat(entry(eng, st, pv, n)) for name, entry in OPEN_LOOP.items()}
            assert all(np.isfinite(c[finite]).all() for c in clean.values())
            for d in pc.deals(clean_params, n, wet, dry, finite, half=coeff == "f16"):
                eng.set_params(d.params, coeff)
                got = {name: _flat(entry(eng, st, pv, n)) for name, entry in OPEN_LOOP.items()}
                for name in OPEN_LOOP:
                    pc.assert_isolated(got[name], clean[name], d.bodies, (name, n))
                dealt_scene, clean_scene = _batch(eng, st, pv, n, beside)
                pc.assert_same_bits(clean_scene, clean["step_wrench_tiled"], (n, "the clean scene of the batch"))
                pc.assert_isolated(dealt_scene, clean["step_wrench_tiled"], d.bodies, (n, "the dealt scene of the batch"))
                with np.errstate(all="ignore"):
                    rule = _cut(pc.device_rule(st, pv, _used(d.params, coeff), RHO, G, DT, semantics), d.bodies)
                    comps_rule = pc.components_rule(st, a32, _used(d.params, coeff), RHO, G, semantics)
                for name in WRENCH:
                    pc.check_rows(got[name][d.bodies], rule, "wrench", d.rows)
                    assert pc.same_bits_or_nan(got[name][d.bodies], got[WRENCH[0]][d.bodies]), (name, n, "the entries differ on a case body")
                pc.check_rows(dealt_scene[d.bodies], rule, "wrench", d.rows)
                assert pc.same_bits_or_nan(dealt_scene[d.bodies], got[WRENCH[0]][d.bodies]), (n, "the batch differs on a case body")
                for name in COMPONENTS:
                    pc.check_rows(got[name][d.bodies], (comps_rule[0][d.bodies], comps_rule[1][d.bodies]), "components", d.rows)
                    assert pc.same_bits_or_nan(got[name][d.bodies], got[COMPONENTS[0]][d.bodies]), (name, n)
                assert pc.same_bits_or_nan(got[SEA_ENTRIES[0]][d.bodies], got[SEA_ENTRIES[1]][d.bodies]), (n, "the sea entries differ on a case body")
                # under a sea: the rule of the state relative to the water, on the case bodies a row is decisive on there too
                under = [i for i, (b, r) in enumerate(zip(d.bodies, d.rows)) if pc._always_reference(r) or (dry_sea[b] if r.dry else wet_sea[b])]
                with np.errstate(all="ignore"):
                    sea_rule = _cut(pc.device_rule(s_rel, pv_rel, _used(d.params, coeff), RHO, G, DT, semantics), d.bodies[under])
                pc.check_rows(got[SEA_ENTRIES[0]][d.bodies[under]], sea_rule, "wrench", [d.rows[i] for i in under])
                under_sea += len(under)
                checked += len(d.bodies)
                deviations += sum(pc.EXPECT[r.name]["wrench"].deviation for r in d.rows)
            eng.set_params(clean_params, coeff)
            again = {name: _flat(entry(eng, st, pv, n)) for name, entry in OPEN_LOOP.items()}
            for name in OPEN_LOOP:
                pc.assert_same_bits(again[name], clean[name], (name, n, "the clean record afterwards"))
        finally:
            eng.set_params(pop["params"][coeff][:n], coeff)
            beside.close()
    print(f"[parameter table, every wrench entry, {coeff} {semantics}] case bodies checked over n = 200 and 321: {checked}, of them rows that "
          f"leave the reference: {deviations}")
    assert checked >= 2 * (len(pc.ROWS) - 6) and deviations >= 2 * len(pc.DEVIATIONS) and under_sea >= 0.9 * checked, (checked, deviations, under_sea)


# ---- 2. the f16 storage ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["numba", "warp"])
def test_the_f16_record_is_the_record_rounded_through_half(semantics, pop, engines):
    rows = 0
    for n in SIZES:
        half, full = engines(n, "f16", semantics), engines(n, "f32", semantics)
        st, pv, (wet, dry, finite) = _population(pop, n)
        clean_params = pop["params"]["f32"][:n]
        try:
            for d in [None] + pc.deals(clean_params, n, wet, dry, finite, half=True):
                raw = clean_params if d is None else d.params
                half.set_params(raw, "f16")
                full.set_params(pc.half_rounded(raw), "f32")
                for name, entry in OPEN_LOOP.items():
                    a, b = _flat(entry(half, st, pv, n)), _flat(entry(full, st, pv, n))
                    assert pc.same_bits_or_nan(a, b), (name, n, "clean" if d is None else "dealt", int((a.view(np.uint32) != b.view(np.uint32)).sum()))
                for implicit in (False, True):
                    outs = []
                    for eng in (half, full):
                        cur, old = _buffers(st, pv, n)
                        outs.append(_from(eng.step_fused_tiled(cur, old, n, DT, implicit_drag=implicit), n))
                    assert pc.same_bits_or_nan(*outs), ("step_fused_tiled", implicit, n, "clean" if d is None else "dealt")
                rows += 0 if d is None else sum(r.group == "half" for r in d.rows)
        finally:
            half.set_params(pop["params"]["f16"][:n], "f16")
            full.set_params(pop["params"]["f32"][:n], "f32")
    assert rows >= 2 * 70                                              # (every edge of the half format, on every coefficient, at both sizes)


# ---- 3. the refusal ---------------------------------------------------------------------------------------------------------------------------
def _c_set_params_f16(eng, params, on_device):
    """hydro_set_params_f16 through the C ABI with host (or device) field arrays; returns (status, message)."""
    soa = np.ascontiguousarray(np.asarray(params, np.float32).T)
    keep = torch.from_numpy(soa).to(DEV) if on_device else soa
    base = keep.data_ptr() if on_device else soa.ctypes.data
    table = nat.pointer_table([base + 4 * f * soa.shape[1] for f in range(nat.PARAM_FIELDS)])
    torch.cuda.synchronize()
    rc = eng._lib.hydro_set_params_f16(eng._h, soa.shape[1], table, int(on_device))
    return rc, eng._lib.hydro_last_error(eng._h).decode()


@pytest.mark.parametrize("start", ["f16", "f32"])
def test_a_coefficient_that_overflows_half_is_refused_and_nothing_is_written(start, pop, engines):
    for n in SIZES:
        eng = engines(n, start)
        st, pv, (wet, _, _) = _population(pop, n)
        clean = pop["params"]["f32"][:n]
        try:
            eng.set_params(clean, start)
            step = lambda: _from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv)), n)  # noqa: E731
            before = step()
            first, second = 70, n - 1                                  # (two offenders: the message names the first body, and its first field)
            assert wet[first]
            for field, value in (("cd_lin", 65520.0), ("damp_lin", 1e5), ("am_ang", -7e4), ("lift", np.float32(3.4e38))):
                bad = clean.copy()
                bad[second, 3:10] = 7e4
                bad[first, pc.FIELDS.index(field)] = value
                bad[first, 9] = bad[first, 9] if field == "am_ang" else 1e6      # a later field of the same body
                assert pc.refused_in_f16(bad).sum() == 2
                with pytest.raises(nat.HydroError) as err:
                    eng.set_params(bad, "f16")
                assert err.value.status == nat.HYDRO_E_ARG
                for rc, message in [(nat.HYDRO_E_ARG, str(err.value))] + [_c_set_params_f16(eng, bad, on_device) for on_device in (0, 1)]:
                    assert rc == nat.HYDRO_E_ARG and f"{field} of body {first}" in message and "hydro_set_params_f32" in message, (rc, message)
                assert eng.coeff_dtype == start and eng.n == n
                pc.assert_same_bits(step(), before, (n, field, "the previous record is still in force"))
            # what is not refused: the largest half, the fp32 number below 65520, NaN and +-Inf given as such, underflow to 0
            fine = clean.copy()
            fine[first, 3:10] = (65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), np.nan, np.inf, -np.inf, 1e-9, -65504.0)
            assert not pc.refused_in_f16(fine).any()
            for on_device in (0, 1):
                rc, message = _c_set_params_f16(eng, fine, on_device)
                assert rc == nat.HYDRO_OK, message
            eng.set_params(fine, "f16")
            assert eng.coeff_dtype == "f16"
            got = step()
            eng.set_params(clean, "f16")
            pc.assert_isolated(got, step(), [first], (n, "the accepted record"))
            assert not np.isfinite(got[first]).all()
        finally:
            eng.set_params(pop["params"][start][:n], start)


# ---- 4. the steps ---------------------------------------------------------------------------------------------------------------------------------
@COEFFS_SEMANTICS
@DRAG
def test_the_single_step_entries_compute_the_constants_as_given(coeff, semantics, implicit, pop, engines):
    worst, held = 0.0, 0
    for n in SIZES:
        eng = engines(n, coeff, semantics)
        st, pv, (wet, dry, finite) = _population(pop, n)
        clean_params = pop["params"]["f32"][:n]

        def fused():
            cur, old = _buffers(st, pv, n)
            w = torch.full((eng.tiles(n), 6, 64), NAN, dtype=torch.float32, device=DEV)
            out = eng.step_fused_tiled(cur, old, n, DT, wrench=w, implicit_drag=implicit)
            return _from(out, n), _from(w, n)

        def integrated(wrench):
            return _from(eng.integrate_tiled(_tiled(st), _tiled(wrench), n, DT), n)
        try:
            eng.set_params(clean_params, coeff)
            clean_state, clean_w = fused()
            clean_int = integrated(clean_w) if not implicit else None
            for d in pc.deals(clean_params, n, wet, dry, finite, half=coeff == "f16"):
                eng.set_params(d.params, coeff)
                state, w = fused()
                pc.assert_isolated(state, clean_state, d.bodies, ("step_fused_tiled", n))
                pc.assert_isolated(w, clean_w, d.bodies, ("step_fused_tiled, the wrench", n))
                hydro = _from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv)), n)
                assert pc.same_bits_or_nan(w[d.bodies], hydro[d.bodies]), (n, "the fused step's wrench is not the wrench entry's")
                with np.errstate(all="ignore"):
                    rule = pc.device_rule(st, pv, _used(d.params, coeff), RHO, G, DT, semantics)
                    k = tuple(x[d.bodies] for x in pc.rule_k(st, d.params, rule[3], coeff)) if implicit else None
                b = d.bodies
                worst = max(worst, pc.check_step(state[b], st[b], hydro[b], d.params[b], k, rule[1][b], io.STEP_ULP_BOUND, G, DT, (n, "fused")))
                for body, r in zip(b, d.rows):                         # what EXPECT says of the row's step, in words, holds too
                    e = pc.EXPECT[r.name]["implicit" if implicit else "explicit"]
                    if e.kind == "reference":
                        assert np.isfinite(state[body]).all(), (r.name, n, state[body])
                    elif e.detail == "all thirteen fields":
                        assert not np.isfinite(state[body]).any(), (r.name, n, state[body])
                if not implicit:                                       # integrate_tiled reads the mass and the dimensions
                    moved = integrated(clean_w)
                    pc.assert_isolated(moved, clean_int, d.bodies, ("integrate_tiled", n))
                    worst = max(worst, pc.check_step(moved[b], st[b], clean_w[b], d.params[b], None, rule[1][b], io.STEP_ULP_BOUND, G, DT, (n, "integrate")))
                held += len(b)
        finally:
            eng.set_params(pop["params"][coeff][:n], coeff)
    print(f"[parameter table, one step, {'implicit' if implicit else 'explicit'} {coeff} {semantics}] worst error of a finite field "
          f"{worst:.2f} ulps (bound {io.STEP_ULP_BOUND:g}) over {held} case bodies")


def _ladder(eng, pop, n, steps, implicit, *, spread, net, chunks=None):
    """The resident ladder's last entry, hydro_step_fused_tiled_multi_spread, with everything on: sea, bed, pose hold, a body-frame
    applied wrench, a three-layer spread, a two-layer net with its link tensions, extremes, every body recorded, ke_out given.
    Per-body arrays as value_contract_launches._everything returns them."""
    eng.set_sea(SEA)
    eng.set_seabed(BED)
    eng.set_watch(list(range(n)))
    cur, old = _buffers(pop["st"], pop["pv"], n)
    record, peaks = _tiled(ex.Extremes.empty(n)), eng.alloc_tiled(2, n)
    sp, nt, ctl, applied = _tiled(spread), _tiled(net), _tiled(pop["ctl"][:n]), _tiled(pop["applied"][:n])
    logs, done = [], 0
    for k in chunks or [steps]:
        log = _log(k, n)
        eng.step_fused_tiled_multi_spread(cur, old, n, DT, k, STEP0 + done, sp, 3, nt, 2, peaks, record, ctl, applied, "body", log=log,
                                          implicit_drag=implicit, ke_out=_ke())
        cur, old = old, cur
        logs.append(_rows(log))
        done += k
    torch.cuda.synchronize()
    rows = np.concatenate(logs)
    return dict(state=_from(cur, n), prev=_from(old, n)[:, 7:13], log=rows.transpose(1, 0, 2).reshape(n, -1), extremes=_from(record, n),
                peaks=_from(peaks, n), statistics=np.zeros((n, 0), np.float32))             # (the spread entry keeps no statistics)


@COEFFS
@DRAG
def test_a_dealt_constant_is_its_bodys_problem_in_the_resident_ladder(coeff, implicit, pop, engines):
    """The spread entry with everything on (`_ladder`), over 1 and 7 steps and as 2 + 5: state, prev_out, log, extremes and peaks of
    every other body have the bits of the launch with the clean record; the case bodies and their partners are untied.  ONE STEP OF
    THE CASE BODIES against integrator_oracle.integrate with the constants as given, as tests/test_mooring_spread_gpu.py forms the
    reference: the device's own wrench of the host-built sea-relative state + the applied wrench + the pose-hold law + the fp64 bed
    wrench + the fp64 sum over the spread's layers (+ the net's: nothing, the bodies are untied), under STEP_ULP_BOUND
    (`check_step`).  Left out of the one step, as there: bodies within 1e-4 of a branch of the hydrodynamic model and the ties with a
    damper; and bodies that touch the bed with a non-positive or non-finite mass or dimension - the contact is fp32 arithmetic with
    a restatement of its own (test_the_seabed_probe_reads_dimensions_and_mass_as_given)."""
    worst, held = 0.0, 0
    for n in SIZES:
        eng = engines(n, coeff)
        st, pv = pop["st"][:n], pop["pv"][:n]
        wet, dry, finite = pc.suitable(st, pv, pop["params"]["f32"][:n])
        clean_params = pop["params"]["f32"][:n]
        spread = np.ascontiguousarray(spread_population(pop["st"], pop["params"]["f32"], pop["moor"])[:n, 0:27])
        eng.set_sea(SEA)
        water = _from(eng.sea_sample(_tiled(st), n, STEP0, DT), n)
        s_rel, pv_rel = sr.relative(st, pv, water[:, 0], water[:, 1:4])
        keep = scenes.branch_margins(s_rel, clean_params) >= 1e-4
        keep[[b for b in (*TIES[4:], *bodies_of(pop["groups"], "ties_c")) if b < n]] = False
        try:
            for d in pc.deals(clean_params, n, wet, dry, finite, half=coeff == "f16", skip_dry=True):
                net = vc.untie(net_for(pop["net"], n, 2), d.bodies)
                vc.assert_untied(net, d.bodies)
                for steps, chunks in ((1, None), (7, None), (7, [2, 5])):
                    run = lambda: _ladder(eng, pop, n, steps, implicit, spread=spread, net=net, chunks=chunks)  # noqa: E731
                    eng.set_params(clean_params, coeff)
                    want = run()
                    eng.set_params(d.params, coeff)
                    got = run()
                    if steps == 1:
                        hydro = _from(eng.step_wrench_tiled(_tiled(s_rel), n, DT, prev=_tiled(pv_rel)), n)
                    eng.set_params(clean_params, coeff)
                    again = run()
                    for key in PER_BODY:
                        pc.assert_isolated(got[key], want[key], d.bodies, (key, n, steps, chunks))
                        pc.assert_same_bits(again[key], want[key], (key, n, steps, chunks, "the clean record afterwards"))
                    assert not vc.same_bits(got["state"][d.bodies], want["state"][d.bodies])
                    if steps != 1:
                        continue
                    b = d.bodies
                    with np.errstate(all="ignore"):
                        rule = pc.device_rule(s_rel, pv_rel, _used(d.params, coeff), RHO, G, DT)
                        k = tuple(x[b] for x in pc.rule_k(s_rel, d.params, rule[3], coeff)) if implicit else None
                        touch = br.touching_fp32(BED, st, d.params)
                        on_m = [mr.taut_fp32(np.ascontiguousarray(rec), st) for rec in msr.layers_of(spread)]
                        on_t = [tr.taut_fp32(rec, st) for rec in tnr.layers_of(net)]
                        extra = br.wrench(BED, st, d.params, touch) + msr.wrench(spread, st, on_m) + tnr.wrench(net, st, on_t)
                        scale = (br.wrench_scales(BED, st, np.abs(np.nan_to_num(d.params)), touch) + msr.wrench_scales(spread, st, on_m)
                                 + tnr.wrench_scales(net, st, on_t))
                        total, surrogate = step_wrench_terms(st[b], hydro[b], applied=pop["applied"][:n][b], frame="body", ctl=pop["ctl"][:n][b],
                                                             bed_wrench=extra[b], bed_scale=np.nan_to_num(scale[b]))
                        odd_bed = ~np.isfinite(extra).all(axis=1) | (touch.any(axis=1) & ~((d.params[:, [0, 1, 2, 10]] > 0).all(axis=1)))
                    skip = rule[1][b] | ~keep[b] | odd_bed[b]
                    worst = max(worst, pc.check_step(got["state"][b], st[b], total, d.params[b], k, skip, io.STEP_ULP_BOUND, G, DT, (n, "ladder"), surrogate))
                    held += int((~skip).sum())
        finally:
            eng.set_sea(None)
            eng.set_seabed(None)
            eng.set_watch(None)
            eng.set_params(pop["params"][coeff][:n], coeff)
    print(f"[parameter table, one step of the spread entry with everything on, {'implicit' if implicit else 'explicit'} {coeff}] worst error of a finite "
          f"field {worst:.2f} ulps (bound {io.STEP_ULP_BOUND:g}) over {held} case bodies")
    assert held >= 150


@COEFFS
def test_the_seabed_probe_reads_dimensions_and_mass_as_given(coeff, pop, engines):
    """Isolation; a coefficient row: the clean bits (the contact reads none); every row of dims and mass against the header's fp32
    operations restated in NumPy (seabed_reference.wrench_fp32_emulated, N = m max(0, .) as given - a negative mass pushes down):
    not finite in the same fields, finite ones within twice PROBE_BOUND of the scale of the constants' magnitudes - device and
    restatement each lie within PROBE_BOUND of the fp64 wrench; a finite positive row also against that fp64 wrench itself."""
    worst = both = 0.0
    rows_held = 0
    for n in SIZES:
        eng = engines(n, coeff)
        st = pop["st"][:n].copy()
        st[:, 2] = (np.float32(BED.z) + np.float32(0.25) * pop["params"]["f32"][:n, 0:3].min(axis=1)).astype(np.float32)   # every box reaches the bed
        wet, dry, finite = pc.suitable(st, pop["pv"][:n], pop["params"]["f32"][:n])
        clean_params = pop["params"]["f32"][:n]
        try:
            eng.set_seabed(BED)
            eng.set_params(clean_params, coeff)
            clean = _from(eng.seabed_wrench(_tiled(st), n), n)
            assert (clean[:, 2] > 0).mean() > 0.9
            for d in pc.deals(clean_params, n, wet, dry, finite, half=coeff == "f16", groups=("dims", "mass", "coefficient"), skip_dry=True):
                eng.set_params(d.params, coeff)
                got = _from(eng.seabed_wrench(_tiled(st), n), n)
                pc.assert_isolated(got, clean, d.bodies, ("hydro_seabed_wrench", n))
                for b, r in zip(d.bodies, d.rows):
                    if pc.FIELDS[r.field] in pc.COEFFS:                  # the contact reads no coefficient
                        pc.assert_same_bits(got[b], clean[b], (r.name, n))
                        continue
                    one = slice(b, b + 1)
                    if pc.EXPECT[r.name]["seabed"].kind == "reference":
                        assert np.isfinite(got[b]).all(), (r.name, n, got[b])
                    if not np.isinf(d.params[b, 0:3]).any():             # the header's fp32 operations as given (an infinite dimension: a
                        with np.errstate(all="ignore"):                 # NaN under max(0, .) is 0 on the device, NaN in NumPy - isolation only)
                            emu = br.wrench_fp32_emulated(BED, st[one], d.params[one])[0].astype(np.float64)
                            mag = np.abs(np.nan_to_num(d.params[one]))
                            size = br.wrench_scales(BED, st[one], mag, br.touching_fp32(BED, st[one], d.params[one]))[0]
                        fin = np.isfinite(emu)
                        assert np.array_equal(np.isfinite(got[b]), fin), (r.name, n, "not finite in other fields than the restatement", got[b], emu)
                        err = np.abs(got[b].astype(np.float64)[fin] - emu[fin]) / (br.ULP * np.where(size[fin] == 0, 1.0, size[fin]))
                        both = max(both, float(err.max(initial=0.0)))
                        assert err.max(initial=0.0) <= 2 * br.PROBE_BOUND, (r.name, n, got[b], emu)
                        rows_held += 1
                    if pc.EXPECT[r.name]["seabed"].kind == "reference" and r.value > 0:
                        touch = br.touching_fp32(BED, st[one], d.params[one])
                        ref, scale = br.wrench(BED, st[one], d.params[one], touch), br.wrench_scales(BED, st[one], d.params[one], touch)
                        err = np.abs(got[one] - ref) / (br.ULP * np.where(scale == 0, 1.0, scale))
                        worst = max(worst, float(err.max()))
                        assert np.isfinite(got[b]).all() and err.max() <= br.PROBE_BOUND, (r.name, n, got[b], ref)
        finally:
            eng.set_seabed(None)
            eng.set_params(pop["params"][coeff][:n], coeff)
    print(f"[parameter table, seabed probe, {coeff}] worst error of a finite positive row {worst:.2f} units of 2^-24 of the scale (bound {br.PROBE_BOUND:g}); "
          f"against the fp32 restatement over {rows_held} rows of dims and mass {both:.2f} (bound {2 * br.PROBE_BOUND:g})")
    assert rows_held >= 2 * 12                                         # (per size: eight rows of dims that are not infinite, four of mass)


# ---- 5. kinetic energy -------------------------------------------------------------------------------------------------------------------------------
def _energy_tables(params, n, wet, dry, finite):
    """(name, params) per launch: the finite rows of dims and mass dealt together, then each non-finite one alone on lane 31."""
    finite_only = params.copy()
    for d in pc.deals(params, n, wet, dry, finite, groups=("dims", "mass"), skip_dry=True):
        for b, r in zip(d.bodies, d.rows):
            if np.isfinite(r.value):
                finite_only[b, r.field] = r.value
    out = [("the finite rows", finite_only)]
    for r in pc.ROWS:
        if r.group in ("dims", "mass") and not np.isfinite(r.value) and not r.dry:
            alone = params.copy()
            alone[31, r.field] = r.value
            out.append((r.name, alone))
    return out


@COEFFS
def test_the_kinetic_energy_entries_sum_every_body_as_given(coeff, pop, engines):
    worst = 0.0
    for n in SIZES:
        eng = engines(n, coeff)
        st, pv = pop["st"][:n], pop["pv"][:n]
        wet, dry, finite = pc.suitable(st, pv, pop["params"]["f32"][:n])
        assert wet[31]
        clean_params = pop["params"]["f32"][:n]
        try:
            tables = _energy_tables(clean_params, n, wet, dry, finite)
            assert len(tables) == 1 + 6 and (tables[0][1][:, pc.MASS] < 0).any()
            assert {name for name, _ in tables[1:]} == {r.name for r in pc.ROWS if pc.EXPECT[r.name]["ke"].kind == "nonfinite" and not r.dry}
            for name, params in tables:
                eng.set_params(params, coeff)
                alone = eng.kinetic_energy(_tiled(st), rotational=True).cpu().numpy()
                sampled = _ke()
                eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv), ke_out=sampled)
                cur, old = _buffers(st, pv, n)
                fused = _ke()
                new = _from(eng.step_fused_tiled(cur, old, n, DT, ke_out=fused), n)
                torch.cuda.synchronize()
                with np.errstate(all="ignore"):
                    cases = (("kinetic_energy", alone, st), ("step_wrench_tiled, ke_out", sampled.cpu().numpy(), st),
                             ("step_fused_tiled, ke_out", fused.cpu().numpy(), new))
                    for entry, got, state in cases:
                        want = scenes.kinetic_energy_fp64(state, params)
                        size = scenes.kinetic_energy_fp64(state, np.abs(params))
                        for g, w, s in zip(got, want, size):
                            if np.isfinite(w):
                                assert np.isfinite(g) and abs(g - w) <= 1e-12 * s, (name, entry, n, g, w)
                                worst = max(worst, abs(g - w) / s if s else 0.0)
                            else:
                                assert not np.isfinite(g), (name, entry, n, g, w)
                    if name == "the finite rows":
                        assert np.isfinite(alone).all() and alone[0] != scenes.kinetic_energy_fp64(st, clean_params)[0]
                    else:
                        assert not np.isfinite(alone).all(), (name, alone)
        finally:
            eng.set_params(pop["params"][coeff][:n], coeff)
    print(f"[parameter table, kinetic energy, {coeff}] worst relative error of a finite sum {worst:.2e} (bound 1e-12)")
