"""The parameter record's value rule (include/hydro.h, "Parameter record") as a table and checkers: what
tests/test_parameter_contract.py shows on the host instantiation of csrc/hydro_body.h and tests/test_parameter_contract_gpu.py asks
of the device.  No device, no library: a checker is a plain function of arrays - the device's output in, an AssertionError out.

THE TABLE (`ROWS`).  One constant of the parameter record - dims(3), the seven coefficients, the mass - changed on a wet, moving
body (`WET_STATE`; `DRY_STATE` is the same body lifted to p_z = +5, for the rows marked `dry`):
  dims (x and z)           -1, -0.0, NaN, +Inf, 1e-20; NaN and +Inf also on the dry body
  each coefficient         -1, -0.0, NaN, +Inf, -Inf
  each coefficient         the edges of the half format (group "half": ordinary numbers in f32 mode) - 65504, the fp32 number below
                           65520, 2^-14, 3e-5 (a subnormal half), 2^-24, 2^-25 (a tie, to 0), the fp32 number above it (to 2^-24),
                           1e-9 (to 0), 1 + 2^-11 (a tie, to 1), 1 + 3 2^-11 (a tie, to 1 + 2^-9)
  cd_lin, damp_lin, am_ang 65520 and 7e4 (group "overflow": hydro_set_params_f16 refuses them, ordinary in f32 mode)
  mass                     -500, NaN, +Inf, 1e-30
The rows of tests/edge_cases.py (zero dims, zero mass, all-zero coefficients) are not repeated.

THE RULE (`device_rule`, `components_rule`): the constants are computed as given.  In fp64, from the oracle's components - which are
the reference's, non-finite constants included (tests/test_oracle_golden.py) - with the four places where the kernels knowingly
leave the reference:
  1. the clamp is fminf(1, m 500 / (|F| + 1e-6)): a NaN factor (a NaN mass, a NaN force) gives 1, the UNCLAMPED wrench - so a
     torque that is finite stays finite beside a NaN force (the reference multiplies everything by the NaN factor);
  2. a factor of exactly 0 (|F| = Inf) wins the product: the wrench is exactly 0 (the reference: 0 x Inf = NaN);
  3. the submersion ratio is fmin(1, .) of the extent: a box with a non-finite dimension has ratio 1 - it is wet wherever it is,
     where the reference sees the keypoints that do not involve the dimension and may call it dry (wrench 0);
  4. a dry body's zeros are selected before any constant is read: its wrench is 0 whatever its coefficients and mass (as in the
     reference, whose early return reads none either).
`EXPECT[row][group]` names, per output group, what kind of answer the row has on the wet (dry) body of the table: `reference`
(finite, held to the fixture and to the oracle), `nonfinite` (which components are not finite) or `exact` (a documented value),
and `deviation` where the device knowingly differs from the reference.  `check_rows` holds a launch's case bodies to the rule.

DEALING (`deal`): the rows go onto bodies of an existing population, whose states stay: lanes 0, 31, 32 and 63 of the first
tile, the first and the last live lane of the last tile, then every third body, at most n // 3 of them (asserted: the isolation
check then covers two thirds of the bodies).  A row that is not `reference` in every group needs a body on which it is decisive
(`suitable`): wet, moving and turning, with area, lift and every component of v, omega and of the accelerations non-zero - or dry,
for the dry rows; any other body takes a finite row.  The table needs several deals (`deals`)."""
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import edge_cases as ec
from oracle import hydro_oracle as ho
from value_contract import assert_isolated, assert_same_bits, _kind  # noqa: F401  (the isolation checker is value_contract's)

FIELDS = ("dim_x", "dim_y", "dim_z", "cd_lin", "cd_ang", "damp_lin", "damp_ang", "lift", "am_lin", "am_ang", "mass")
COEFFS = FIELDS[3:10]
MASS = 10
RHO, G, DT = ec.RHO, ec.G, ec.DT
WET_STATE = np.array([0.0, 0.0, -0.2, 0.1, 0.2, 0.05, 0.97, 0.3, -0.1, 0.5, 0.2, 0.1, -0.4], np.float32)
DRY_STATE = np.array([0.0, 0.0, 5.0, 0.1, 0.2, 0.05, 0.97, 0.3, -0.1, 0.5, 0.2, 0.1, -0.4], np.float32)
PREV = np.array([0.25, -0.05, 0.4, 0.1, 0.2, -0.3], np.float32)
CLEAN = np.array([1.0, 0.8, 0.6] + ec.STD + [500.0], np.float32)
GROUPS = ("wrench", "components", "explicit", "implicit", "ke", "seabed")

Row = namedtuple("Row", "name field value dry group")

HALF_EDGES = (("65504", 65504.0, 65504.0), ("below 65520", np.nextafter(np.float32(65520.0), np.float32(0)), 65504.0),
              ("2^-14", 2.0 ** -14, 2.0 ** -14), ("3e-5", 3e-5, 2.0 ** -24 * 503), ("2^-24", 2.0 ** -24, 2.0 ** -24), ("2^-25", 2.0 ** -25, 0.0),
              ("above 2^-25", np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -24), ("1e-9", 1e-9, 0.0),
              ("1 + 2^-11", 1.0 + 2.0 ** -11, 1.0), ("1 + 3 2^-11", 1.0 + 3.0 * 2.0 ** -11, 1.0 + 2.0 ** -9))     # (name, fp32 value, its half)
OVERFLOW_FIELDS = ("cd_lin", "damp_lin", "am_ang")
HALF_MAX_ROUNDS_UP = 65520.0                                       # the smallest magnitude __float2half_rn stores as Inf


def _rows():
    rows = []
    for f in ("dim_x", "dim_z"):
        for tag, v in (("-1", -1.0), ("-0", -0.0), ("NaN", np.nan), ("+Inf", np.inf), ("1e-20", 1e-20)):
            rows.append(Row(f"{f} = {tag}", FIELDS.index(f), np.float32(v), False, "dims"))
            if tag in ("NaN", "+Inf"):
                rows.append(Row(f"{f} = {tag} [dry]", FIELDS.index(f), np.float32(v), True, "dims"))
    for f in COEFFS:
        for tag, v in (("-1", -1.0), ("-0", -0.0), ("NaN", np.nan), ("+Inf", np.inf), ("-Inf", -np.inf)):
            rows.append(Row(f"{f} = {tag}", FIELDS.index(f), np.float32(v), False, "coefficient"))
    for f in COEFFS:
        for tag, v, _ in HALF_EDGES:
            rows.append(Row(f"{f} = {tag}", FIELDS.index(f), np.float32(v), False, "half"))
    for f in OVERFLOW_FIELDS:
        for tag, v in (("65520", 65520.0), ("7e4", 7e4)):
            rows.append(Row(f"{f} = {tag}", FIELDS.index(f), np.float32(v), False, "overflow"))
    for tag, v in (("-500", -500.0), ("NaN", np.nan), ("+Inf", np.inf), ("1e-30", 1e-30)):
        rows.append(Row(f"mass = {tag}", MASS, np.float32(v), False, "mass"))
    return tuple(rows)


ROWS = _rows()
NAMES = [r.name for r in ROWS]
ROW = {r.name: r for r in ROWS}


def half_rounded(params):
    """The record the f16 mode computes with: the seven coefficients through numpy's half (round to nearest even)."""
    out = np.array(params, np.float32)
    with np.errstate(over="ignore"):
        out[..., 3:10] = out[..., 3:10].astype(np.float16).astype(np.float32)
    return out


def refused_in_f16(params):
    """(n,) bool: hydro_set_params_f16 refuses the record - a FINITE coefficient of magnitude >= 65520."""
    c = np.abs(np.asarray(params, np.float32)[..., 3:10])
    with np.errstate(invalid="ignore"):
        return (np.isfinite(c) & (c >= np.float32(HALF_MAX_ROUNDS_UP))).any(axis=-1)


def table():
    """(names, state, prev, params) of the fixture: every row on the body of the docstring, and after them the half rows once more
    with the coefficient already rounded to half (name + ' [as half]'): what the f16 mode computes with."""
    names, state, params = [], [], []
    for r in ROWS:
        p = CLEAN.copy()
        p[r.field] = r.value
        names.append(r.name)
        state.append(DRY_STATE if r.dry else WET_STATE)
        params.append(p)
    for r in ROWS:
        if r.group == "half":
            p = CLEAN.copy()
            p[r.field] = r.value
            names.append(r.name + " [as half]")
            state.append(WET_STATE)
            params.append(half_rounded(p))
    n = len(names)
    return names, np.array(state, np.float32), np.tile(PREV, (n, 1)), np.array(params, np.float32)


def reference_outputs():
    """tests/golden/parameter_cases.npz: what the REFERENCE ITSELF returns for `table()` (make_golden.py --only-params); refuses a
    fixture that was made for another version of the table."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parameter_cases.npz"))
    names, state, prev, params = table()
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731  (NaN rows: by bits)
    assert [str(x) for x in z["names"]] == names and same(z["state"], state) and same(z["prev"], prev) and same(z["params"], params), \
        "parameter_cases.npz is stale: python3 -B tests/golden/make_golden.py --only-params"
    return {k: z[k] for k in z.files}


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def _value_class(v):
    return "nan" if np.isnan(v) else ("finite" if np.isfinite(v) else ("+inf" if v > 0 else "-inf"))


Expectation = namedtuple("Expectation", "kind detail deviation why")
REFERENCE = Expectation("reference", None, False, "")
ALL6 = (True,) * 6
FORCE, TORQUE = (True, True, True, False, False, False), (False, False, False, True, True, True)


def _expect_wrench(r):
    """The net wrench (F | T) of the row on the table's own body."""
    cls, f = _value_class(r.value), FIELDS[r.field]
    if cls == "finite":
        return REFERENCE
    if f.startswith("dim"):
        # rule 3: ratio = fmin(1, NaN) = 1 and a non-finite volume; the reference agrees but for the NaN dimension on the dry body,
        # where it sees only the finite keypoints and returns zeros (an infinite dimension puts keypoints at z = -Inf: wet there too)
        return Expectation("nonfinite", ALL6, r.dry and cls == "nan", "the ratio of a box with a non-finite dimension is fmin(1, NaN) = 1: wet wherever it is")
    if f == "mass":
        if cls == "nan":
            return Expectation("exact", "unclamped", True, "the clamp's fminf(1, NaN) = 1: the unclamped wrench")
        return REFERENCE                                               # +Inf: a factor of +Inf, min(1, .) = 1 in the reference too
    if f in ("cd_lin", "damp_lin", "lift"):
        if cls == "nan":
            return Expectation("nonfinite", ALL6, False, "")
        return Expectation("exact", "zero", True, "|F| = Inf makes the clamp factor 0, and 0 wins the product (v_mul_legacy_f32)")
    if f in ("cd_ang", "damp_ang"):                                    # the force does not read them; the torque takes the clamp factor of the force
        return Expectation("nonfinite", TORQUE, False, "")
    if f == "am_ang":
        return Expectation("nonfinite", TORQUE, False, "")
    assert f == "am_lin"
    if cls == "nan":
        return Expectation("nonfinite", FORCE, True, "the clamp's fminf(1, NaN) = 1: the torque does not pass through the force's NaN")
    # +-Inf: R (kf R^T a) mixes infinities of both signs; with a NaN among them the factor is 1 and the torque stays finite,
    # without one |F| = Inf and the whole wrench is 0: `device_rule` says which, per body
    return Expectation("nonfinite", None, True, "an infinite force: a NaN factor is 1 (the torque stays), a zero factor wins (the wrench is 0)")


def _expect_components(r):
    cls, f = _value_class(r.value), FIELDS[r.field]
    if cls == "finite" or f == "mass":
        return REFERENCE                                               # (the calculator surface does not read the mass)
    if f.startswith("dim"):
        return Expectation("nonfinite", "ratio 1; buoyancy z, and for a NaN the drag torque, both added-mass vectors and both centres",
                           True, "the ratio of a box with a non-finite dimension is fmin(1, NaN) = 1")
    which = {"cd_lin": "drag_force", "damp_lin": "drag_force", "lift": "lift_force", "cd_ang": "drag_torque", "damp_ang": "drag_torque",
             "am_lin": "added_mass_force", "am_ang": "added_mass_torque"}[f]
    return Expectation("nonfinite", which, False, "")


def _expect_step(r):
    """One closed-loop step: io.integrate of the row's own wrench with the row's own constants - finite where that is finite and
    within fp32, not finite in the same fields where it is not."""
    w = _expect_wrench(r)
    if FIELDS[r.field] == "mass" and np.isinf(r.value):
        return Expectation("nonfinite", "all thirteen fields", True,
                           "1 / m is a hardware seed and a Newton step: 0 + 0 (1 - Inf x 0) = NaN, where fp64 division gives 0")
    return Expectation("reference" if w.kind == "reference" and np.isfinite(r.value) else w.kind, "integrate", w.deviation, w.why)


def _expect_ke(r):
    f = FIELDS[r.field]
    if np.isfinite(r.value) or f in COEFFS:
        return REFERENCE                                               # 1/2 m |v|^2 (+ the box inertia): no coefficient in it
    return Expectation("nonfinite", "the sum over all bodies", False, "")


def _expect_seabed(r):
    f = FIELDS[r.field]
    if np.isfinite(r.value) or f in COEFFS:
        return REFERENCE                                               # the contact reads dims and mass only
    return Expectation("nonfinite", "as the fp64 restatement", False, "")


EXPECT = {r.name: {"wrench": _expect_wrench(r), "components": _expect_components(r), "explicit": _expect_step(r), "implicit": _expect_step(r),
                   "ke": _expect_ke(r), "seabed": _expect_seabed(r)} for r in ROWS}
DEVIATIONS = tuple(r.name for r in ROWS if EXPECT[r.name]["wrench"].deviation)


def _net(state, comps):
    p = np.asarray(state, np.float64)[:, 0:3]
    arm_b, arm_p = comps["center_of_buoyancy"] - p, comps["center_of_pressure"] - p
    net_f = comps["buoyancy_force"] + comps["drag_force"] + comps["lift_force"] + comps["added_mass_force"]
    net_t = (np.cross(arm_b, comps["buoyancy_force"]) + np.cross(arm_p, comps["drag_force"]) + np.cross(arm_p, comps["lift_force"])
             + comps["drag_torque"] + comps["added_mass_torque"])
    return net_f, net_t


def device_rule(state, prev, params, rho=RHO, g=G, dt=DT, semantics="numba"):
    """(W (n, 6) float64, or_zero (n,) bool, unclamped (n, 6), comps): the header's rule for the net wrench.  W: the oracle's
    components summed and clamped as the header says - a NaN factor is 1, a zero factor wins; a box with a NaN dimension: NaN in
    all six; `or_zero` where a dimension is infinite: no component is finite (each +-Inf or NaN, by the body's attitude), or -
    where the infinities leave |F| = Inf without a NaN - the factor is 0 and the whole wrench is 0."""
    state, params = np.asarray(state, np.float32), np.asarray(params, np.float32)
    with np.errstate(all="ignore"):
        accel = ho.finite_difference_accel(state, prev, dt)
        comps = ho.solve_components(state, accel, params.astype(np.float64), rho, g, semantics)
        net_f, net_t = _net(state, comps)
        unclamped = np.concatenate([net_f, net_t], axis=1)
        factor = params[:, MASS].astype(np.float64) * ho.MAX_ACCEL / (np.linalg.norm(net_f, axis=1) + ho.CLAMP_EPS)
        s = np.where(factor < 1.0, factor, 1.0)                        # fminf(1, NaN) = 1
        W = unclamped * s[:, None]
        W[s == 0.0] = 0.0                                              # 0 wins the product, whatever the other operand
        W[comps["ratio"] == 0.0] = 0.0                                 # a dry body: zeros, whatever its mass
    bad = ~np.isfinite(params[:, 0:3]).all(axis=1)
    W[bad] = np.nan
    comps["scale"] = np.where(bad, np.nan, s)
    return W, np.isinf(params[:, 0:3]).any(axis=1), unclamped, comps


def components_rule(state, accel, params, rho=RHO, g=G, semantics="numba"):
    """(want (n, 25) float64, checked (n, 25) bool): the calculator surface - eight vectors and the ratio - of the oracle at the
    constants as given; for a non-finite dimension what the header states and no more: ratio 1, buoyancy (0, 0, +Inf or NaN), and
    for a NaN dimension NaN in the drag torque, both added-mass vectors and both centres."""
    params = np.asarray(params, np.float32)
    with np.errstate(all="ignore"):
        c = ho.solve_components(np.asarray(state, np.float32), np.asarray(accel, np.float64), params.astype(np.float64), rho, g, semantics)
    want = np.concatenate([c[f] for f in ho.COMPONENT_FIELDS] + [c["ratio"][:, None]], axis=1)
    checked = np.ones(want.shape, bool)
    nan_dim, inf_dim = np.isnan(params[:, 0:3]).any(axis=1), np.isinf(params[:, 0:3]).any(axis=1)
    bad = nan_dim | inf_dim
    checked[bad] = False
    want[bad, 24], checked[bad, 24] = 1.0, True
    want[bad, 0:2], checked[bad, 0:2] = 0.0, True
    want[bad, 2], checked[bad, 2] = np.where(nan_dim[bad], np.nan, np.inf), True
    only_nan = nan_dim & ~inf_dim
    turning = np.linalg.norm(np.asarray(state, np.float64)[:, 10:13], axis=1) > ho.SPEED_EPS
    for k in (3, 4, 5, 6, 7):                                          # drag torque (of a turning body), added-mass force and torque, cob, cop
        rows = only_nan & turning if k == 3 else only_nan
        want[rows, 3 * k:3 * k + 3], checked[rows, 3 * k:3 * k + 3] = np.nan, True
    return want, checked


def suitable(state, prev, params, rho=RHO, g=G, dt=DT):
    """(wet (n,), dry (n,), finite (n,)) bool: the bodies of a population on which every wet (dry) row is decisive, by the oracle on
    the clean constants - see the module's docstring - and those whose own state is finite: no other body takes a row at all."""
    state, prev = np.asarray(state, np.float32), np.asarray(prev, np.float32)
    with np.errstate(all="ignore"):
        _, _, c = ho.step_wrench(state, prev, params, rho, g, dt)
    v, w = state[:, 7:10].astype(np.float64), state[:, 10:13].astype(np.float64)
    moving = (np.linalg.norm(v, axis=1) > 1e-3) & (np.linalg.norm(w, axis=1) > 1e-3) & (np.abs(state[:, 7:13]) > 0).all(axis=1)
    accel = (np.abs(state[:, 7:13].astype(np.float64) - prev) > 0).all(axis=1)
    lifted = np.linalg.norm(c["lift_force"], axis=1) > 0
    finite = np.isfinite(state).all(axis=1) & np.isfinite(prev).all(axis=1)
    wet = finite & (c["ratio"] > 1e-3) & (c["area"] > 1e-3) & moving & accel & lifted & (np.asarray(params)[:, MASS] > 0)
    dry = finite & (c["ratio"] == 0.0) & (state[:, 2] > 4.0 * np.abs(np.asarray(params)[:, 0:3]).sum(axis=1))
    return wet, dry, finite


def case_bodies(n):
    """The bodies that carry a row: lanes 0, 31, 32, 63 of the first tile, the first and the last live lane of the last tile (at
    n = 321 they are one body: lane 0 of the tile in front and body n - 2 as well), then every third body up to n // 3 in all."""
    first = 64 * ((n - 1) // 64)
    must = [0, 31, 32, 63, first, n - 1] + ([first - 64, n - 2] if first == n - 1 else [])
    must = [b for b in dict.fromkeys(must) if 0 <= b < n]
    rest = [b for b in range(1, n, 3) if b not in must]
    return must, rest, n // 3


def _always_reference(r):
    return all(e.kind == "reference" for e in EXPECT[r.name].values())


def deals(params, n, wet, dry, finite=None, half=False, groups=None, skip_dry=False):
    """The table dealt onto the first n bodies of a population, in as many deals as it takes: a list of namespaces with params
    (n, 11) float32, clean (the population's own), bodies (k,), rows (k Rows).  half: the f16 mode - the overflow rows are left
    out (hydro_set_params_f16 refuses them).  groups: only the rows of these groups.  skip_dry: without the dry rows (a population
    that has no dry body)."""
    clean = np.array(params[:n], np.float32)
    pending = [r for r in ROWS if (groups is None or r.group in groups) and not (half and r.group == "overflow") and not (skip_dry and r.dry)]
    safe = [r for r in ROWS if _always_reference(r) and not (half and r.group == "overflow")]
    must, rest, cap = case_bodies(n)
    assert len(must) <= cap
    out, spare = [], 0

    def fits(r, b):
        return (finite is None or finite[b]) and (_always_reference(r) or (dry[b] if r.dry else wet[b]))
    while pending:
        p, bodies, rows, took = clean.copy(), [], [], 0
        for b in must + rest:
            if len(bodies) == cap or (not pending and b not in must):
                break
            r = next((r for r in pending if fits(r, b)), None)
            if r is not None:
                pending.remove(r)
                took += 1
            elif b in must:                                           # the lane carries a row all the same: a finite one, in turn
                assert finite is None or finite[b], b
                r, spare = safe[spare % len(safe)], spare + 1
            else:
                continue
            p[b, r.field] = r.value
            bodies.append(b)
            rows.append(r)
        assert 3 * len(bodies) <= n, (len(bodies), n)                  # the isolation check covers at least two thirds of the bodies
        assert took, f"no body of the population suits the rows {[r.name for r in pending][:4]}"
        out.append(SimpleNamespace(params=p, clean=clean, bodies=np.array(bodies), rows=rows))
    return out


def deal(params, n, wet=None, dry=None, finite=None, **kw):
    """The first deal (every lane the module's docstring names carries a row); `deals` gives all of them."""
    everybody = np.ones(n, bool)
    return deals(params, n, everybody if wet is None else wet, ~everybody if dry is None else dry, finite, **kw)[0]


# ---- the checkers -----------------------------------------------------------------------------------------------------------------------
def _tolerances(W):
    """edge_cases.check's: 1e-6 of the body's largest term, per body (n, 6)."""
    W = np.nan_to_num(np.abs(W), nan=0.0, posinf=0.0, neginf=0.0)
    tol_f = 1e-6 * np.maximum(1.0, W[:, 0:3].max(axis=1))
    tol_t = 1e-6 * np.maximum(1.0, W.max(axis=1))
    return np.concatenate([np.repeat(tol_f[:, None], 3, axis=1), np.repeat(tol_t[:, None], 3, axis=1)], axis=1)


def check_rows(got, expect, group, rows=None):
    """`got` (k, F): the device's output for the k case bodies of a deal; `expect`: what `device_rule` (group "wrench": the tuple it
    returns, cut to the case bodies) or `components_rule` (group "components": (want, checked)) gives for them; rows: their Rows.
    Finite expectation: edge_cases.check's tolerance (centres: half an fp32 ulp).  Non-finite: the same class - NaN, +Inf, -Inf -
    component by component.  An exact zero is an exact zero.  Where EXPECT states which components are not finite, exactly those are."""
    got = np.asarray(got, np.float64)
    if group == "wrench":
        want, or_zero = np.asarray(expect[0], np.float64), np.asarray(expect[1], bool)
        assert got.shape == want.shape, (got.shape, want.shape)
        tol = _tolerances(want)
        for i in range(len(got)):
            name = rows[i].name if rows is not None else i
            if or_zero[i]:                                             # an infinite dimension: every component +-Inf or NaN - or, where
                assert not got[i].any() or not np.isfinite(got[i]).any(), (name, got[i])    # |F| = Inf without a NaN, the factor 0 won
                continue
            fin = np.isfinite(want[i])
            assert np.array_equal(_kind(got[i]), _kind(want[i])), (name, got[i], want[i])
            assert (np.abs(got[i][fin] - want[i][fin]) <= tol[i][fin]).all(), (name, got[i], want[i])
            if not want[i].any() and fin.all():                     # a dry body, a zero factor: exact zeros
                assert not got[i].any(), (name, "exactly zero", got[i])
            if rows is not None:
                e = EXPECT[rows[i].name]["wrench"]
                if e.kind == "nonfinite" and e.detail is not None:
                    assert np.array_equal(~np.isfinite(got[i]), np.array(e.detail)), (name, "the components that are not finite", got[i])
                if e.kind == "exact" and e.detail == "zero":
                    assert not got[i].any(), (name, "exactly zero", got[i])
                if e.kind in ("reference", "exact"):
                    assert np.isfinite(got[i]).all(), (name, got[i])
        return
    assert group == "components", group
    want, checked = np.asarray(expect[0], np.float64), np.asarray(expect[1], bool)
    assert got.shape == want.shape == (len(got), 25), (got.shape, want.shape)
    for i in range(len(got)):
        name = rows[i].name if rows is not None else i
        c = checked[i]
        assert np.array_equal(_kind(got[i])[c], _kind(want[i])[c]), (name, got[i], want[i])
        fin = c & np.isfinite(want[i])
        scale = max(1.0, np.abs(np.where(np.isfinite(want[i][:18]), want[i][:18], 0.0)).max())
        tol = np.full(25, 1e-6 * scale)
        centres = np.where(np.isfinite(want[i][18:24]), want[i][18:24], 0.0)
        tol[18:24] = 0.5 * np.spacing(np.abs(centres).astype(np.float32)).astype(np.float64) * (1 + 1e-6) + 1e-12
        tol[24] = 1e-6
        assert (np.abs(got[i][fin] - want[i][fin]) <= tol[fin]).all(), (name, got[i], want[i])
        if rows is not None:
            e = EXPECT[rows[i].name]["components"]
            if e.kind == "reference":
                assert np.isfinite(got[i]).all(), (name, got[i])
            elif e.detail in ho.COMPONENT_FIELDS:                      # a coefficient: its own vector and nothing else
                k = ho.COMPONENT_FIELDS.index(e.detail)
                bad = ~np.isfinite(got[i])
                assert bad[3 * k:3 * k + 3].any() and not np.delete(bad, range(3 * k, 3 * k + 3)).any(), (name, got[i])


def same_bits_or_nan(a, b):
    """Equal bit for bit, a NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- one closed-loop step ------------------------------------------------------------------------------------------------------------------
STEP_FIELDS = {"position": slice(0, 3), "quaternion": slice(3, 7), "velocity": slice(7, 10), "angular_velocity": slice(10, 13)}
QUATERNION_RATE_MAX = 1e17                                         # (the square of dt / 2 times a rate beyond ~1e19 rad/s overflows fp32, and the norm with it)
INSIDE_FP32, FP32_MAX = 1e30, 3.5e38                               # a field of the fp64 step is held to the bound below the first, asked to be not finite above the second


def rule_k(state, params, comps, coeff="f32", rho=RHO):
    """(k_lin, k_ang) of the implicit form by the rule: integrator_oracle.drag_jacobian with the rule's clamp factor, and 0 where
    the factor is 0 or the body dry - the zero wins the product there too (hydro_body.h assemble_wrench)."""
    from oracle import integrator_oracle as io
    with np.errstate(all="ignore"):
        k_lin, k_ang = io.drag_jacobian(state, params, {c: comps[c] for c in ("ratio", "area", "scale")}, rho, coeff)
    zero = (comps["scale"] == 0.0) | (comps["ratio"] == 0.0)
    return np.where(zero, 0.0, k_lin), np.where(zero, 0.0, k_ang)


def check_step(got, state, hydro, params, k, skip, bound, g=G, dt=DT, what="", surrogate=None):
    """One step of the case bodies against integrator_oracle.integrate of the device's own fp32 hydrodynamic wrench `hydro`, with
    the constants as given.  Per field group: where the fp64 result is finite and inside fp32 range, within `bound` (in units of
    2^-24 of integrator_oracle.field_scales, formed from the MAGNITUDES of the constants: a negative mass is a term like any
    other); a component that is not finite, or beyond fp32, is not finite on the device.  Two things the magnitudes do not say:
      - the implicit form divides by m - dt k_lin and I_a - dt k_ang, which a negative constant (a negative volume makes k_ang
        positive) lets CANCEL: the fp32 rounding of the two terms is amplified by (|m| + dt |k|) / |m - dt k|, and so are the
        scales here - the factor is 1 for constants of the ordinary signs;
      - 1 / m, 1 / I_a and the implicit denominators are a hardware seed and one Newton step, r + r (1 - x r): for x = +-Inf the
        seed is 0 and the step is 0 x Inf = NaN, where fp64 division gives 0.  A body with an INFINITE MASS therefore leaves the
        step with NaN in all thirteen fields (fp64: a finite explicit step under gravity alone).
    skip (k,) bool: bodies of which only isolation is asked (an infinite dimension).  surrogate: what the scales are formed from
    in place of `hydro` where `hydro` is a sum of terms that may cancel (resident_harness.step_wrench_terms).  Returns the worst
    error of the groups held to the bound."""
    from oracle import integrator_oracle as io
    got, hydro = np.asarray(got, np.float64), np.asarray(hydro, np.float64)
    clean = lambda a: np.nan_to_num(np.asarray(a, np.float64), nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
    with np.errstate(all="ignore"):
        ref = io.integrate(state, hydro, params, g, dt, *(k or (None, None)))
        scales = io.field_scales(state, clean(hydro if surrogate is None else surrogate), np.abs(clean(params)), g, dt, None if k is None else tuple(clean(x) for x in k), clean(ref))
        if k is not None:
            m, inertia = np.asarray(params, np.float64)[:, 10], io.box_inertia(params)
            kl, ka = np.asarray(k[0], np.float64), np.asarray(k[1], np.float64)[:, None]
            amp_lin = clean((np.abs(m) + dt * np.abs(kl)) / np.abs(m - dt * kl))[:, None]
            amp_ang = clean((np.abs(inertia) + dt * np.abs(ka)) / np.abs(inertia - dt * ka))
            qn = np.linalg.norm(np.asarray(state, np.float64)[:, 3:7], axis=1)
            scales["velocity"] = scales["velocity"] * amp_lin
            scales["position"] = np.abs(np.asarray(state, np.float64)[:, 0:3]) + dt * scales["velocity"]
            scales["angular_velocity"] = scales["angular_velocity"] * amp_ang.max(axis=1, keepdims=True)
            scales["quaternion"] = qn * (1.0 + 0.5 * dt * np.linalg.norm(scales["angular_velocity"], axis=1))
        err = io.integrator_error_ulps(got, ref, state, hydro, params, g, dt, k, scales=scales)
    worst = 0.0
    infinite_mass = np.isinf(np.asarray(params, np.float64)[:, 10])
    for i in range(len(got)):
        if skip[i]:
            continue
        if infinite_mass[i]:
            assert not np.isfinite(got[i]).any(), (what, i, "an infinite mass: NaN in all thirteen fields", got[i])
            continue
        for group, c in STEP_FIELDS.items():
            r, d = ref[i, c], got[i, c]
            with np.errstate(invalid="ignore"):
                outside = ~np.isfinite(r) | (np.abs(r) > FP32_MAX)
                inside = np.isfinite(r) & (np.abs(r) < INSIDE_FP32)
                if group == "quaternion":                              # |q + dt/2 (w', 0) q|^2 is formed in fp32: beyond |w'| ~ 1e19 it overflows
                    inside = inside & bool(np.all(np.abs(ref[i, 10:13]) < QUATERNION_RATE_MAX))
            assert not np.isfinite(d[outside]).any(), (what, i, group, "finite where the fp64 step is not", d, r)
            if inside.all():
                assert np.isfinite(d).all(), (what, i, group, "not finite where the fp64 step is", d, r)
                e = float(err[group][i])
                worst = max(worst, e)
                assert e <= bound, (what, i, group, e, bound, d, r)
    return worst
