"""The parameter record's rule (include/hydro.h; tests/parameter_cases.py) on the host: the table is what it claims, the host
instantiation of csrc/hydro_body.h (tests/host_emul/emul.cpp) meets `check_rows` on the table's own body and on the dealt
population, the rows marked `deviation` are exactly those on which it leaves the reference's own answers
(tests/golden/parameter_cases.npz), and the checkers fail on mutations of the expected output.

WHERE THE EMULATION IS NOT THE DEVICE.  emul.cpp has libm's division and square root where the kernels have the hardware seeds
and a Newton step; on the rows of this table the two agree in kind: 1 / Inf is +0 and 1 / NaN is NaN either way, the seed of +Inf
is +0 and the Newton step of a zero seed of an INFINITE argument is fma(0, NaN, 0) = NaN where libm gives 0 - and both reach the
same fmin(1, NaN) = 1 from there (the ratio of a box with an infinite dimension).  tests/test_parameter_contract_gpu.py holds
the device to the same `check_rows`; a row on which the two differed would be listed here."""
import ctypes
import os

import numpy as np
import pytest

import parameter_cases as pc
import value_contract as vc
from conftest import REPO
from designed_populations import bed_pop, hold_pop  # noqa: F401  (fixtures are requested by name)
from value_contract_launches import pop  # noqa: F401  (a fixture)

SEMANTICS = ("numba", "warp")


@pytest.fixture(scope="module")
def emul(native_built):
    """(wrench, components) of the host instantiation: fp32 arrays (n, 6) and (n, 25)."""
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "host_emul", "libemul.so"))
    fp = ctypes.POINTER(ctypes.c_float)
    ptr = lambda a: a.ctypes.data_as(fp)  # noqa: E731

    def wrench(state, prev, params, semantics="numba"):
        n = len(state)
        f, t, r = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        st, pv, pr = (np.ascontiguousarray(x, np.float32) for x in (state, prev, params))
        lib.emul_set_semantics(int(semantics == "warp"))
        try:
            assert lib.emul_wrench(ctypes.c_int64(n), ptr(st), ptr(pv), ptr(pr), ctypes.c_double(pc.RHO), ctypes.c_double(pc.G),
                                   ctypes.c_double(pc.DT), ptr(f), ptr(t), ptr(r)) == 0
        finally:
            lib.emul_set_semantics(0)
        return np.concatenate([f, t], axis=1)

    def components(state, accel, params, semantics="numba"):
        n = len(state)
        out, r = np.empty((n, 8, 3), np.float32), np.empty(n, np.float32)
        st, ac, pr = (np.ascontiguousarray(x, np.float32) for x in (state, accel, params))
        lib.emul_set_semantics(int(semantics == "warp"))
        try:
            assert lib.emul_components(ctypes.c_int64(n), ptr(st), ptr(ac), ptr(pr), ctypes.c_double(pc.RHO), ctypes.c_double(pc.G), ptr(out), ptr(r)) == 0
        finally:
            lib.emul_set_semantics(0)
        return np.concatenate([out.reshape(n, 24), r[:, None]], axis=1)
    return wrench, components


def _accel32(state, prev):
    with np.errstate(all="ignore"):
        return ((state[:, 7:13] - prev) / np.float32(pc.DT)).astype(np.float32)


def _cut(rule, idx):
    return tuple(np.asarray(a)[idx] for a in rule[:3])


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_one_the_rule_speaks_of():
    groups = {g: sum(r.group == g for r in pc.ROWS) for g in ("dims", "coefficient", "half", "overflow", "mass")}
    assert groups == dict(dims=14, coefficient=35, half=70, overflow=6, mass=4) and len(set(pc.NAMES)) == len(pc.ROWS)
    assert sum(r.dry for r in pc.ROWS) == 4
    with np.errstate(over="ignore"):
        for tag, value, as_half in pc.HALF_EDGES:                      # numpy's half is the round-to-nearest-even the header names
            assert float(np.float32(value).astype(np.float16)) == as_half, tag
        assert np.isinf(np.float32(65520.0).astype(np.float16)) and np.isinf(np.float32(7e4).astype(np.float16))
    below = np.nextafter(np.float32(65520.0), np.float32(0))
    assert below < 65520.0 and float(below.astype(np.float16)) == 65504.0
    assert float(np.float32(3e-5).astype(np.float16)) < 2.0 ** -14      # a subnormal half
    names, state, prev, params = pc.table()
    refused = pc.refused_in_f16(params)
    assert [n for n, r in zip(names, refused) if r] == [r.name for r in pc.ROWS if r.group == "overflow"]
    assert not pc.refused_in_f16(pc.half_rounded(params[~refused])).any()
    kinds = {g: {pc.EXPECT[n][g].kind for n in pc.NAMES} for g in pc.GROUPS}
    assert kinds["wrench"] == {"reference", "nonfinite", "exact"} and all(k <= {"reference", "nonfinite", "exact"} for k in kinds.values())
    assert len(pc.DEVIATIONS) == 2 + 6 + 3 + 1                         # NaN dims dry; cd_lin, damp_lin, lift +-Inf; am_lin NaN, +-Inf; mass NaN


@pytest.mark.parametrize("n", vc.SIZES)
def test_dealing(n, pop):
    z = pop["zero"]
    wet, dry, finite = pc.suitable(z["st"][:n], z["pv"][:n], pop["params"]["f32"][:n])
    assert wet.sum() >= n // 2 and dry.sum() >= 8 and (~finite).sum() == 2
    for half in (False, True):
        all_deals = pc.deals(pop["params"]["f32"], n, wet, dry, finite, half=half)
        dealt = [r.name for d in all_deals for r in d.rows]
        want = [r.name for r in pc.ROWS if not (half and r.group == "overflow")]
        assert set(want) <= set(dealt) and (not half or not set(dealt) & {r.name for r in pc.ROWS if r.group == "overflow"})
        first = 64 * ((n - 1) // 64)
        for d in all_deals:
            assert 3 * len(d.bodies) <= n and len(set(d.bodies)) == len(d.bodies)
            assert {0, 31, 32, 63, first, n - 1} <= set(d.bodies.tolist())
            others = ~np.isin(np.arange(n), d.bodies)
            assert vc.same_bits(d.params[others], d.clean[others]) and others.sum() >= 2 * n / 3
            for b, r in zip(d.bodies, d.rows):                             # one constant of the body's own record, nothing else
                changed = d.params[b].view(np.uint32) != d.clean[b].view(np.uint32)
                assert not np.delete(changed, r.field).any(), (b, r.name)
                assert finite[b] and ((dry[b] if r.dry else wet[b]) or pc._always_reference(r)), (b, r.name)
            if half:
                assert not pc.refused_in_f16(d.params).any()


# ---- the host instantiation on the table's own body -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", SEMANTICS)
def test_the_host_instantiation_meets_the_table_on_its_own_body(semantics, emul):
    wrench, components = emul
    names, state, prev, params = pc.table()
    k = len(pc.ROWS)                                                   # (behind them: the half rows already rounded - finite, `reference`)
    rows = list(pc.ROWS) + [pc.ROW[n[:-len(" [as half]")]] for n in names[k:]]
    with np.errstate(all="ignore"):
        got = wrench(state, prev, params, semantics)
        pc.check_rows(got, pc.device_rule(state, prev, params, semantics=semantics), "wrench", rows)
        a32 = _accel32(state, prev)
        pc.check_rows(components(state, a32, params, semantics), pc.components_rule(state, a32, params, semantics=semantics), "components", rows)
    # the deviations include/hydro.h lists, on this body
    at = names.index
    assert np.isnan(got[at("dim_x = NaN")]).all() and np.isnan(got[at("dim_x = NaN [dry]")]).all() and np.isnan(got[at("dim_z = +Inf")]).all()
    for f in ("cd_lin", "damp_lin", "lift"):
        assert not got[at(f"{f} = +Inf")].any() and not got[at(f"{f} = -Inf")].any()
    for tag in ("NaN", "+Inf"):
        g = got[at(f"am_lin = {tag}")]
        assert not np.isfinite(g[0:3]).any() and np.isfinite(g[3:6]).all() and g[3:6].any()
    assert np.isfinite(got[at("mass = NaN")]).all()


def test_the_deviations_are_the_rows_on_which_the_host_instantiation_leaves_the_reference(emul):
    """Against the reference's own answers: a row is marked `deviation` exactly if its net wrench differs IN KIND from the fixture's;
    every other row is held to the fixture - finite values at edge_cases.check's tolerance, the same NaNs and infinities.  An
    infinite dimension: whether a component is an infinity or a NaN is the body's attitude's affair in either; "not finite" is compared."""
    wrench, _ = emul
    fx = pc.reference_outputs()
    names, state, prev, params = pc.table()
    with np.errstate(all="ignore"):
        got = wrench(state, prev, params).astype(np.float64)
    ref = np.concatenate([fx["net_force"], fx["net_torque"]], axis=1)
    tol = pc._tolerances(ref)
    differ = []
    for i, name in enumerate(names):
        infinite_dim = np.isinf(params[i, 0:3]).any()
        if not np.array_equal(*((np.isfinite(got[i]), np.isfinite(ref[i])) if infinite_dim else (vc._kind(got[i]), vc._kind(ref[i])))):
            differ.append(name)
            continue
        fin = np.isfinite(ref[i])
        assert (np.abs(got[i][fin] - ref[i][fin]) <= tol[i][fin]).all(), (name, got[i], ref[i])
    assert differ == list(pc.DEVIATIONS), (differ, pc.DEVIATIONS)
    assert all(pc.EXPECT[n]["wrench"].why for n in pc.DEVIATIONS)


# ---- the host instantiation on the dealt population ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("coeff", ["f32", "f16"])
def test_the_host_instantiation_meets_the_table_on_the_dealt_population(coeff, semantics, pop, emul):
    wrench, components = emul
    z = pop["zero"]
    checked = 0
    for n in vc.SIZES:
        st, pv = z["st"][:n], z["pv"][:n]
        wet, dry, finite = pc.suitable(st, pv, pop["params"]["f32"][:n])
        used = lambda p: pc.half_rounded(p) if coeff == "f16" else p  # noqa: E731  (what the f16 mode computes with)
        a32 = _accel32(st, pv)
        for d in pc.deals(pop["params"]["f32"], n, wet, dry, finite, half=coeff == "f16"):
            with np.errstate(all="ignore"):
                clean_w, got_w = wrench(st, pv, used(d.clean), semantics), wrench(st, pv, used(d.params), semantics)
                clean_c, got_c = components(st, a32, used(d.clean), semantics), components(st, a32, used(d.params), semantics)
                pc.assert_isolated(got_w, clean_w, d.bodies, (n, "wrench"))
                pc.assert_isolated(got_c, clean_c, d.bodies, (n, "components"))
                rule = pc.device_rule(st, pv, used(d.params), semantics=semantics)
                pc.check_rows(got_w[d.bodies], _cut(rule, d.bodies), "wrench", d.rows)
                want, which = pc.components_rule(st, a32, used(d.params), semantics=semantics)
                pc.check_rows(got_c[d.bodies], (want[d.bodies], which[d.bodies]), "components", d.rows)
            checked += len(d.bodies)
    assert checked >= 2 * len(pc.ROWS) - 12


# ---- the checkers fail on mutations ---------------------------------------------------------------------------------------------------------
def test_the_checkers_fail_on_mutations_of_the_expected_output(emul):
    wrench, components = emul
    names, state, prev, params = pc.table()
    k = len(pc.ROWS)
    state, prev, params, rows = state[:k], prev[:k], params[:k], list(pc.ROWS)
    with np.errstate(all="ignore"):
        got = wrench(state, prev, params)
        rule = pc.device_rule(state, prev, params)
        pc.check_rows(got, rule, "wrench", rows)
        at = names.index
        # zeros accepted where NaN is expected
        bad = got.copy()
        bad[at("cd_lin = NaN")] = 0.0
        with pytest.raises(AssertionError):
            pc.check_rows(bad, rule, "wrench", rows)
        # a finite torque accepted where the whole wrench must be NaN
        bad = got.copy()
        bad[at("dim_x = NaN"), 3:6] = (1.0, -2.0, 0.5)
        with pytest.raises(AssertionError):
            pc.check_rows(bad, rule, "wrench", rows)
        # a NaN torque accepted where the torque must stay finite beside the NaN force; a NaN where the zero factor wins
        for name, cols in (("am_lin = NaN", slice(3, 6)), ("damp_lin = +Inf", slice(0, 6)), ("mass = NaN", slice(0, 1))):
            bad = got.copy()
            bad[at(name), cols] = np.nan
            with pytest.raises(AssertionError):
                pc.check_rows(bad, rule, "wrench", rows)
        # a finite row off by more than the tolerance; the clamped wrench where the unclamped one is expected
        bad = got.copy()
        bad[at("cd_ang = -1"), 4] *= np.float32(1.001)
        with pytest.raises(AssertionError):
            pc.check_rows(bad, rule, "wrench", rows)
        a32 = _accel32(state, prev)
        comps, crule = components(state, a32, params), pc.components_rule(state, a32, params)
        pc.check_rows(comps, crule, "components", rows)
        bad = comps.copy()
        bad[at("lift = NaN"), 3:6] = np.nan                            # the drag force of a row that may only lose its lift
        with pytest.raises(AssertionError):
            pc.check_rows(bad, crule, "components", rows)
    # one non-case body moved by one bit
    clean = np.arange(600, dtype=np.float32).reshape(100, 6)
    moved = clean.copy()
    moved[[3, 40]] = np.nan                                            # the case bodies may hold anything
    pc.assert_isolated(moved, clean, [3, 40])
    moved[41, 2] = np.nextafter(moved[41, 2], np.float32(np.inf))
    with pytest.raises(AssertionError):
        pc.assert_isolated(moved, clean, [3, 40])


def test_the_unclamped_row_is_seen(emul):
    """mass = NaN on a body whose clean wrench IS clamped: the rule's expectation is the unclamped wrench, and the clamped one fails."""
    wrench, _ = emul
    state, prev = pc.WET_STATE[None, :].copy(), pc.PREV[None, :].copy()
    state[0, 7:10] = (30.0, -20.0, 10.0)                               # fast: |F| >> m 500
    light, nan_mass = pc.CLEAN[None, :].copy(), pc.CLEAN[None, :].copy()
    light[0, pc.MASS], nan_mass[0, pc.MASS] = 0.5, np.nan
    with np.errstate(all="ignore"):
        clamped, free = wrench(state, prev, light), wrench(state, prev, nan_mass)
        rule = pc.device_rule(state, prev, nan_mass)
        assert np.linalg.norm(clamped[0, :3]) < 0.5 * np.linalg.norm(free[0, :3])
        pc.check_rows(free, rule, "wrench", [pc.ROW["mass = NaN"]])
        with pytest.raises(AssertionError):
            pc.check_rows(clamped, rule, "wrench", [pc.ROW["mass = NaN"]])
