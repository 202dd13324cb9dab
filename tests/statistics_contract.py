"""The value rules of include/hydro.h, "Statistics", as tables and checkers: what tests/test_statistics_contract.py shows on the
host and tests/test_statistics_contract_gpu.py asks of the device.  No device, no library: every function here is a plain function of
arrays.  The comparison is always `check_record`: every word of a record equals `statistics.fold`, bit for bit.

WHY THIS MODULE.  That comparison has teeth only where the mistakes the header forbids change a bit.  With a level within a few
ulps of the sample (or 0, or a short number) d = x - L has few significant bits, d * d is exact in fp64, and a contracted
fma(d, d, S2), an fp32 difference (Sterbenz) or another order of addition give the bits of the header's arithmetic: the test cannot
fail.  So:

1. GAP LEVELS (`gap_levels`): levels 5 to 12 binary orders below the sample with a full random mantissa.  d then has 29 to 36
   significant bits, d * d is inexact, every addition rounds.
2. MUTATIONS (`fold_fused` .. `fold_pairwise`): `fold` with exactly one rule broken, each formed exactly (the fused sum through
   fractions.Fraction).  `_variant` without a mutation is an independent restatement of `fold`.
3. LEVEL ROWS (`level_table`): NaN, +-Inf, -0 and +0 against samples of +0, the smallest denormal of both signs, +-3e38, the sample
   of step k itself and its two neighbours - dealt over value_contract.poisoned_bodies' lanes and every fifth body, never more than
   a third of the population; every other body keeps its gap level.
4. SEED ROWS (`seeded_record`): the record a launch starts from - sums of -0, NaNs of both signs (one with a payload), +-Inf,
   1e300 and full-mantissa values of the samples' own magnitude and of 2^40 times it; up-words 0x80000000, 0x7fffffff, 0xffffffff,
   0xfffffffe; n words 0xffffffff, 0xfffffffd, 0x80000000.
5. `assert_rows_cover`: the meetings the tables are about really occur in the samples of a launch.  Returns the counts.
"""
from fractions import Fraction

import numpy as np

import value_contract as vc
from silver2_isaacsim_amd import statistics as stx

F32, F64, U32 = np.float32, np.float64, np.uint32
FALLBACK_LEVEL = np.array([0x3A9D4953], U32).view(F32)[0]          # 1.2e-3 with a full mantissa (the low bit is set)
PAYLOAD_NAN = np.array([0x7ff8000000001234], np.uint64).view(F64)[0]
NEGATIVE_NAN = np.array([0xfff8000000000000], np.uint64).view(F64)[0]
DENORMAL = np.array([0x00000001], U32).view(F32)[0]
# the caps: conditions on the INPUTS, asserted on the host reference first and on the device's rows second
FUSED_CAP, FP32_DIFFERENCE_CAP, SEEDED_CAP, LEVEL_ROWS_CAP = 0.25, 0.5, 0.25, 1.0 / 3.0


def _bits32(a):
    return np.ascontiguousarray(a, F32).view(U32)


def first_nonzero(samples):
    """(n,): per body the first sample of (steps, n) that is not 0 (0 where there is none)."""
    s = np.asarray(samples, F32)
    k = np.argmax(s != 0, axis=0)
    return s[k, np.arange(s.shape[1])]


# ---- 1. gap levels ----------------------------------------------------------------------------------------------------------------------
def gap_levels(samples0, seed):
    """(n, 2) fp32 levels for the (n, 2) first samples of the two slots: 5 to 12 binary orders below the sample's magnitude, a full
    random mantissa (the low bit set), a random sign; FALLBACK_LEVEL where the sample is 0, denormal or not finite."""
    s = np.asarray(samples0, F32)
    assert s.ndim == 2 and s.shape[1] == 2
    rng = np.random.default_rng(seed)
    mantissa = rng.integers(0, 1 << 23, s.shape).astype(U32) | U32(1)
    drop = rng.integers(5, 13, s.shape).astype(np.int64)
    sign = rng.integers(0, 2, s.shape).astype(U32) << U32(31)
    e = ((_bits32(s) >> U32(23)) & U32(0xff)).astype(np.int64)
    ok = np.isfinite(s) & (e - drop >= 1)
    lev = (sign | (np.where(ok, e - drop, 1).astype(U32) << U32(23)) | mantissa).view(F32)
    return np.where(ok, lev, FALLBACK_LEVEL).astype(F32)


def designed_gap_levels(samples_a, samples_b, seed, tries=4):
    """Gap levels for the (steps, n) samples of the two slots, below each body's first non-zero sample, DESIGNED like every table here:
    of `tries` draws of `gap_levels` a (body, slot) pair keeps the first under which a fused S2 differs from fold's over those
    samples (the first draw where none does).  A fused sum shows on about three pairs in ten of one random draw - the later steps'
    rounding hides most of it behind the growing sum -, which is too near the cap of a quarter to be left to chance."""
    a, b = np.asarray(samples_a, F32), np.asarray(samples_b, F32)
    s0 = np.stack([first_nonzero(a), first_nonzero(b)], axis=1)
    lev = gap_levels(s0, seed)
    settled = np.zeros(lev.shape, bool)
    for t in range(tries):
        cand = gap_levels(s0, seed + 7919 * t)
        for c, xs in enumerate((a, b)):
            idx = np.flatnonzero(~settled[:, c])
            if not len(idx):
                continue
            two = np.stack([cand[idx, c], cand[idx, c]], axis=1)
            shows = s2_differs(fold_fused(None, xs[:, idx], xs[:, idx], two), stx.fold(None, xs[:, idx], xs[:, idx], two))[:, 0]
            lev[idx[shows], c] = cand[idx[shows], c]
            settled[idx[shows], c] = True
    return lev


def orders_below(samples0, levels):
    """floor(log2 |x|) - floor(log2 |L|) per (body, slot); NaN where either is 0 or not finite."""
    s, lev = np.asarray(samples0, F64), np.asarray(levels, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.floor(np.log2(np.abs(s))) - np.floor(np.log2(np.abs(lev)))
    return np.where(np.isfinite(out), out, np.nan)


# ---- 2. fold, restated, and its exact mutations -----------------------------------------------------------------------------------------
def _fma_rows(d, s2):
    """round(s2 + d * d), ONE rounding, per element: exact in fractions.Fraction; where an operand is not finite or the exact sum is
    zero (the sign of a zero is IEEE's business) the plain two-rounding arithmetic, which cannot differ there."""
    with np.errstate(invalid="ignore", over="ignore"):
        out = s2 + d * d
    for i in np.flatnonzero(np.isfinite(d) & np.isfinite(s2)):
        exact = Fraction(float(d[i])) * Fraction(float(d[i])) + Fraction(float(s2[i]))
        if exact != 0:
            try:
                out[i] = float(exact)
            except OverflowError:
                out[i] = np.inf if exact > 0 else -np.inf
    return out


def _variant(record, samples_a, samples_b, levels, *, fused=False, fp32_difference=False, ge=False, unmasked_count=False, nan_above=False,
             pairwise=False):
    """include/hydro.h's arithmetic, restated apart from statistics.fold, with at most one rule broken."""
    a, b, lev = np.asarray(samples_a, F32), np.asarray(samples_b, F32), np.asarray(levels, F32)
    n = a.shape[1]
    assert a.ndim == 2 and a.shape == b.shape and lev.shape == (n, 2)
    rec = stx.empty(n) if record is None else record
    sums, up = np.array(rec["sums"], F64), np.array(rec["up"], U32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, xs in enumerate((a, b)):
            L32 = lev[:, c]
            L = L32.astype(F64)
            p1, p2 = np.zeros(n), np.zeros(n)
            for x in xs:
                d = (x - L32).astype(F64) if fp32_difference else x.astype(F64) - L
                q = d * d
                if pairwise:
                    p1, p2 = p1 + d, p2 + q
                else:
                    sums[:, 2 * c] = sums[:, 2 * c] + d
                    sums[:, 2 * c + 1] = _fma_rows(d, sums[:, 2 * c + 1]) if fused else sums[:, 2 * c + 1] + q
                above = (x >= L32) if ge else ~(x <= L32) if nan_above else (x > L32)
                w = up[:, c]
                step = (w >> U32(31)) & above.astype(U32)
                count = ((w & stx.COUNT_MASK) + step) if unmasked_count else ((w + step) & stx.COUNT_MASK)
                up[:, c] = count | np.where(above, U32(0), stx.LAST_BELOW)
            if pairwise:
                sums[:, 2 * c], sums[:, 2 * c + 1] = sums[:, 2 * c] + p1, sums[:, 2 * c + 1] + p2
    cnt = ((np.asarray(rec["n"], U32).astype(np.uint64) + np.uint64(a.shape[0])) & np.uint64(0xffffffff)).astype(U32)
    return {"sums": sums, "up": up, "n": cnt}


def fold_restated(record, samples_a, samples_b, levels):
    return _variant(record, samples_a, samples_b, levels)


def fold_fused(record, samples_a, samples_b, levels):
    """S2 = round(S2 + d * d): one rounding (a contracted fma)."""
    return _variant(record, samples_a, samples_b, levels, fused=True)


def fold_fp32_difference(record, samples_a, samples_b, levels):
    """d = float64(float32(x - L))."""
    return _variant(record, samples_a, samples_b, levels, fp32_difference=True)


def fold_ge(record, samples_a, samples_b, levels):
    """above = x >= L."""
    return _variant(record, samples_a, samples_b, levels, ge=True)


def fold_unmasked_count(record, samples_a, samples_b, levels):
    """The count's carry is allowed into bit 31."""
    return _variant(record, samples_a, samples_b, levels, unmasked_count=True)


def fold_nan_above(record, samples_a, samples_b, levels):
    """above = not (x <= L): true for a NaN."""
    return _variant(record, samples_a, samples_b, levels, nan_above=True)


def fold_pairwise(record, samples_a, samples_b, levels):
    """S1 and S2 of a launch are summed apart, from +0, and added to the record once.  (Over ONE step from any record this IS the
    header's arithmetic - 0 + d is d -: the mutation shows from the second step of a launch on.)"""
    return _variant(record, samples_a, samples_b, levels, pairwise=True)


MUTATIONS = {"fused": fold_fused, "fp32_difference": fold_fp32_difference, "ge": fold_ge, "unmasked_count": fold_unmasked_count,
             "nan_above": fold_nan_above, "pairwise": fold_pairwise}


def s2_differs(a, b):
    """(n, 2) bool: S2 of slot a, b differs in bits (a NaN equals a NaN)."""
    x, y = np.asarray(a["sums"], F64)[:, 1::2], np.asarray(b["sums"], F64)[:, 1::2]
    return (np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64)) & ~(np.isnan(x) & np.isnan(y))


def body_differs(a, b):
    """(n,) bool: any word of the body's record differs (a NaN sum equals a NaN sum)."""
    x, y = np.asarray(a["sums"], F64), np.asarray(b["sums"], F64)
    sums = (np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64)) & ~(np.isnan(x) & np.isnan(y))
    return sums.any(axis=1) | (np.asarray(a["up"], U32) != np.asarray(b["up"], U32)).any(axis=1) | (np.asarray(a["n"], U32) != np.asarray(b["n"], U32))


def finite_pairs(samples_a, samples_b, levels):
    """(n, 2) bool: every sample of the slot and its level are finite."""
    lev = np.asarray(levels, F32)
    return np.stack([np.isfinite(np.asarray(s, F32)).all(axis=0) for s in (samples_a, samples_b)], axis=1) & np.isfinite(lev)


def live_pairs(samples_a, samples_b, levels):
    """finite_pairs, less the pairs with fewer than two samples that are not 0 (on the tension channel: a body whose line pulls in
    one step at most): where x = 0, d = -L is a number of 24 bits whose square is exact, and the one inexact square is added to a sum
    of exact ones - NO level makes a fused S2 show there.  They are not part of the population the caps speak of."""
    return finite_pairs(samples_a, samples_b, levels) & np.stack([(np.asarray(s, F32) != 0).sum(axis=0) >= 2 for s in (samples_a, samples_b)], axis=1)


def assert_gap_caps(samples_a, samples_b, levels, what="", least=64):
    """The conditions on a launch from the EMPTY record with gap levels: fold_fused differs from fold in S2 on at least FUSED_CAP of
    the finite (body, slot) pairs (`live_pairs`) and fold_fp32_difference on at least FP32_DIFFERENCE_CAP.  Returns the fractions."""
    want = stx.fold(None, samples_a, samples_b, levels)
    finite = live_pairs(samples_a, samples_b, levels)
    assert finite.sum() >= least, (what, "too few finite pairs", int(finite.sum()))   # (explicit drag carries most of a population without a pose hold away)
    fused = float(s2_differs(fold_fused(None, samples_a, samples_b, levels), want)[finite].mean())
    narrow = float(s2_differs(fold_fp32_difference(None, samples_a, samples_b, levels), want)[finite].mean())
    assert fused >= FUSED_CAP and narrow >= FP32_DIFFERENCE_CAP, (what, fused, narrow)
    return dict(fused=fused, fp32_difference=narrow, finite_pairs=int(finite.sum()))


def assert_seeded_caps(samples_a, samples_b, levels, seed, what=""):
    """The conditions on a launch from the SEEDED record, on the bodies that carry a full-mantissa seed (and whose samples and levels
    are finite in the steps looked at): fold_fused differs from fold after the FIRST step on at least SEEDED_CAP of them, and fold_pairwise - which is the
    header's arithmetic over one step - over the whole launch, which must then have two steps or more."""
    a, b = np.asarray(samples_a, F32), np.asarray(samples_b, F32)
    first = full_mantissa_bodies(len(seed["n"])) & finite_pairs(a[:1], b[:1], levels).all(axis=1)
    full = first & finite_pairs(a, b, levels).all(axis=1)
    assert first.sum() >= 8 and full.sum() >= 4, (what, int(first.sum()), int(full.sum()))
    one = stx.fold(seed, a[:1], b[:1], levels)
    fused = float(body_differs(fold_fused(seed, a[:1], b[:1], levels), one)[first].mean())
    assert not body_differs(fold_pairwise(seed, a[:1], b[:1], levels), one).any(), what
    assert len(a) >= 2, what
    pairwise = float(body_differs(fold_pairwise(seed, a, b, levels), stx.fold(seed, a, b, levels))[full].mean())
    assert fused >= SEEDED_CAP and pairwise >= SEEDED_CAP, (what, fused, pairwise)
    return dict(fused=fused, pairwise=pairwise, bodies=int(first.sum()), finite_to_the_end=int(full.sum()))


# ---- 3. level rows ----------------------------------------------------------------------------------------------------------------------
LEVEL_ROWS = ("nan", "+inf", "-inf", "denormal", "-denormal", "+3e38", "-3e38", "sample", "sample_up", "sample_down")
ZERO_BODIES = vc.ZERO_BODIES[:6]                                   # x, y and the tension are +0 there: -0 and +0 levels in turn
INF_BODIES = (*vc.INF_BODIES, *vc.ZERO_BODIES[6:8])                # 138: x = +Inf, 139: y = -Inf; 136 and 137 made the same by `more_infinities`


def more_infinities(st):
    """value_contract.exact_zero_bodies' state with two more dry bodies at infinity, 136 at x = +Inf and 137 at y = -Inf: one of each
    kind meets a finite level, the other its own infinity."""
    st = np.array(st, F32)
    st[vc.ZERO_BODIES[6], 0], st[vc.ZERO_BODIES[7], 1] = np.inf, -np.inf
    return st


def dealt_bodies(n):
    """The bodies that take a level row: value_contract.poisoned_bodies(n)'s lanes and every fifth body."""
    return np.unique(np.concatenate([vc.poisoned_bodies(n), np.arange(2, n, 5)]))


def level_table(samples_a, samples_b, seed, zero_bodies=()):
    """((n, 2) fp32 levels, (n, 2) the name of each level's row, '' for a gap level) from the (steps, n) samples of the two slots.
    Gap levels everywhere; LEVEL_ROWS in turn over `dealt_bodies` (slot b three rows ahead of slot a; 'sample' is the sample of step
    body % steps); -0 and +0 in turn on `zero_bodies` (ZERO_BODIES for the designed
    population, whose INF_BODIES are skipped too); and where a slot's first sample is infinite, the same infinity on every other such body (the others keep the finite fallback level)."""
    a, b = np.asarray(samples_a, F32), np.asarray(samples_b, F32)
    steps, n = a.shape
    lev = gap_levels(np.stack([a[0], b[0]], axis=1), seed)
    names = np.full((n, 2), "", dtype=object)
    fixed = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "denormal": DENORMAL, "-denormal": -DENORMAL, "+3e38": 3e38, "-3e38": -3e38}
    for c, xs in enumerate((a, b)):
        for i, body in enumerate(dealt_bodies(n)):
            if len(zero_bodies) and (body in vc.ZERO_BODIES or body in INF_BODIES):
                continue
            name = LEVEL_ROWS[(i + 3 * c) % len(LEVEL_ROWS)]
            x = xs[body % steps, body]
            value = fixed[name] if name in fixed else x if name == "sample" else np.nextafter(x, F32(np.inf if name == "sample_up" else -np.inf))
            lev[body, c], names[body, c] = value, name
        for i, body in enumerate(zero_bodies):
            lev[body, c], names[body, c] = (-0.0, "-0") if i % 2 == 0 else (0.0, "+0")
        for i, body in enumerate(np.flatnonzero(np.isinf(xs[0]))):
            if i % 2 == 0:
                lev[body, c], names[body, c] = xs[0, body], "same_infinity"
    assert (names != "").any(axis=1).mean() <= LEVEL_ROWS_CAP, float((names != "").any(axis=1).mean())
    return lev.astype(F32), names


# ---- 4. seed rows -----------------------------------------------------------------------------------------------------------------------
SUM_SEEDS = ("-0", "payload_nan", "full", "negative_nan", "+inf", "full", "-inf", "1e300", "full")
UP_SEEDS = (0x80000000, 0x7fffffff, 0xffffffff, 0xfffffffe)
N_SEEDS = (0xffffffff, 0xfffffffd, 0x80000000)


def _sum_kind(n):
    kind = np.full(n, "", dtype=object)
    bodies = np.arange(1, n, 3)
    kind[bodies] = [SUM_SEEDS[i % len(SUM_SEEDS)] for i in range(len(bodies))]
    return kind


def full_mantissa_bodies(n):
    """(n,) bool: the bodies whose four sums are seeded with full-mantissa values."""
    return _sum_kind(n) == "full"


def seeded_record(samples0, seed):
    """statistics.empty(n) with, on dealt bodies (every third body from 1 the sums, every fourth from 2 the up-words, every seventh
    from 3 the n word): SUM_SEEDS in turn in all four sums - 'full': in one slot S1 a full-mantissa value of the first sample's
    magnitude and S2 one of its square's, NEGATIVE (within a quarter of what d * d adds, so that the first addition cancels two bits
    or more and keeps the low bits a fused sum would not have rounded away: a seed is any double), in the other slot 2^40 times those
    magnitudes, the slots in turn, so every addition rounds -, UP_SEEDS in turn (slot b one ahead of slot a), N_SEEDS in turn.  `samples0`: (n, 2) the first samples."""
    s0 = np.asarray(samples0, F64)
    n = len(s0)
    rng = np.random.default_rng(seed)
    rec = stx.empty(n)
    mag = np.where(np.isfinite(s0) & (np.abs(s0) > 1e-30) & (np.abs(s0) < 1e30), np.abs(s0), 1.0)
    fixed = {"-0": -0.0, "payload_nan": PAYLOAD_NAN, "negative_nan": NEGATIVE_NAN, "+inf": np.inf, "-inf": -np.inf, "1e300": 1e300}
    kind = _sum_kind(n)
    for i, body in enumerate(np.flatnonzero(kind != "")):
        if kind[body] != "full":
            rec["sums"][body, :] = fixed[kind[body]]
            continue
        for c in range(2):
            big = 2.0 ** 40 if (i + c) % 2 else 1.0
            m = rng.uniform(1.0, 2.0, 2) * rng.choice([-1.0, 1.0])
            rec["sums"][body, 2 * c] = big * m[0] * mag[body, c]
            rec["sums"][body, 2 * c + 1] = 2.0 ** 40 * abs(m[1]) * mag[body, c] ** 2 if (i + c) % 2 else -rng.uniform(0.75, 1.25) * mag[body, c] ** 2
    ups = np.arange(2, n, 4)
    for c in range(2):
        rec["up"][ups, c] = [UP_SEEDS[(i + c) % len(UP_SEEDS)] for i in range(len(ups))]
    ns = np.arange(3, n, 7)
    rec["n"][ns] = [N_SEEDS[i % len(N_SEEDS)] for i in range(len(ns))]
    return rec


# ---- 5. the checks ----------------------------------------------------------------------------------------------------------------------
MEETINGS = ("nan_sample", "+inf_finite_level", "-inf_finite_level", "+inf_same_infinity", "-inf_same_infinity", "equal_not_zero",
            "+0_against_-0", "wrap_of_0xffffffff", "n_wraps", "finite_after_nan")


def assert_rows_cover(samples_a, samples_b, levels, seed, require=MEETINGS):
    """The meetings the tables are about, counted over both slots of one launch from `seed` (the dict of statistics.empty) and
    asserted for those named in `require` (a launch has two channels: no pair holds a +Inf and a -Inf sample).  Returns the counts."""
    lev = np.asarray(levels, F32)
    counts = dict.fromkeys(MEETINGS, 0)
    steps = len(samples_a)
    for c, xs in enumerate((np.asarray(samples_a, F32), np.asarray(samples_b, F32))):
        L = lev[:, c][None, :]
        fin = np.isfinite(L)
        counts["nan_sample"] += int(np.isnan(xs).sum())
        counts["+inf_finite_level"] += int((np.isposinf(xs) & fin).sum())
        counts["-inf_finite_level"] += int((np.isneginf(xs) & fin).sum())
        counts["+inf_same_infinity"] += int((np.isposinf(xs) & np.isposinf(L)).sum())
        counts["-inf_same_infinity"] += int((np.isneginf(xs) & np.isneginf(L)).sum())
        counts["equal_not_zero"] += int(((xs == L) & (xs != 0)).sum())
        counts["+0_against_-0"] += int(((_bits32(xs) == 0) & (_bits32(np.broadcast_to(L, xs.shape)) == U32(0x80000000))).sum())
        # the word seeded 0xffffffff counts - and wraps to 0 - with the first sample above its level
        with np.errstate(invalid="ignore"):
            counts["wrap_of_0xffffffff"] += int(((np.asarray(seed["up"], U32)[:, c] == U32(0xffffffff)) & (xs[0] > lev[:, c])).sum())
        nan = np.isnan(xs)
        counts["finite_after_nan"] += int((np.maximum.accumulate(nan, axis=0)[:-1] & np.isfinite(xs[1:])).sum()) if steps > 1 else 0
    counts["n_wraps"] = int((np.asarray(seed["n"], U32).astype(np.uint64) + np.uint64(steps) > np.uint64(0xffffffff)).sum())
    missing = [m for m in require if not counts[m]]
    assert not missing, (missing, counts)
    return counts


def same_record(a, b):
    """statistics_reference.same_record: bit for bit, a NaN sum equal to a NaN sum whatever its payload."""
    return not body_differs(a, b).any()


def check_record(got, samples_a, samples_b, levels, seed, what="", fold=stx.fold):
    """Every word of `got` equals fold(seed, ...) bit for bit (a NaN sum equals a NaN sum whatever its payload).  `fold` is
    statistics.fold; a test of THIS function passes a mutation in its place."""
    want = fold(seed, samples_a, samples_b, levels)
    differ = body_differs(got, want)
    assert not differ.any(), (what, int(differ.sum()), np.flatnonzero(differ)[:8].tolist())
    return want
