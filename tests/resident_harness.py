"""What the GPU tests of the resident closed-loop entries share: the sizes, launch lengths and parametrisations, the tile
strides of the guard tests that have one value everywhere, the small device helpers, ONE engine caller (`step`), ONE caller of
the C ABI (`raw`) and ONE error measure against the fp64 step (`fp64_step_errors`).  A new resident option adds a row to
`ENTRIES` and `RAW_EXTRAS` and a term to `fp64_step_errors`; it does not copy a test module.

Strides that differ between modules (the extremes record's, the probes') stay in their modules: the guard tests test them.
"""
import ctypes

import numpy as np
import pytest
import torch

import populations
import pose_hold_reference as phr
import sea_reference as sr
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd.engine import HydroEngine

DEV = "cuda:0"
B = io.STEP_ULP_BOUND
SIZES = (1, 63, 64, 65, 257, 4097)
STEPS = (1, 2, 7)
FRAMES = ("world", "body")
RHO, G, DT = populations.RHO, populations.G, populations.DT
NAN = float("nan")
COEFFS = pytest.mark.parametrize("coeff", ["f32", "f16"])
DRAG = pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
# the chain tests (device against device, bit for bit) hold in either semantics: the Numba cases keep their ids
COEFFS_SEMANTICS = pytest.mark.parametrize("coeff,semantics", [("f32", "numba"), ("f16", "numba"), ("f32", "warp"), ("f16", "warp")],
                                           ids=["f32", "f16", "f32-warp", "f16-warp"])
S_IN, S_OUT, S_PV, S_PVO, S_A = 13 * 64 + 36, 13 * 64 + 100, 6 * 64 + 20, 6 * 64 + 12, 6 * 64 + 28
VIEW_STEPS = (0, 1, 7, 10 ** 6)                                   # the steps the sea is sampled at
S_C = 17 * 64 + 44                                               # the control record's tile stride in the guard tests
S_M = 9 * 64 + 52                                                 # the mooring record's


def _tiled(x):
    return torch.from_numpy(scenes.to_tiled(x)).to(DEV)


def _engine(n, params, coeff, semantics="numba"):
    eng = HydroEngine(n, DEV, RHO, G)
    eng.set_params(params[:n], coeff)
    if semantics != "numba":
        eng.set_semantics(semantics)
    return eng


def _buffers(st, pv, n):
    """(cur, old): the state and the buffer whose velocity fields hold the previous velocity, as ClosedLoopSim keeps them."""
    old = np.zeros((n, 13), np.float32)
    old[:, 7:13] = pv[:n]
    return _tiled(st[:n]), _tiled(old)


def _ke():
    return torch.full((2,), NAN, dtype=torch.float64, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_values(a, b):
    """torch.equal that lets a NaN equal a NaN: the explicit form may carry a light, strongly damped body of the population
    out of the fp32 range within seven steps, with or without an applied wrench."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _from(t, n):
    return scenes.from_tiled(t.contiguous().cpu().numpy(), n)


def _watched(n, bodies=(0, 5, 63, 64, 130)):
    """The watched bodies of a launch of n: those of `bodies` that exist, and the last one."""
    return sorted({b for b in (*bodies, n - 1) if b < n})


def _rows(log):
    """(rows, 19, n) device log -> (rows, n, 19) host."""
    return np.ascontiguousarray(log.cpu().numpy().transpose(0, 2, 1))


def _log(rows, n):
    return torch.full((rows, 19, n), NAN, dtype=torch.float32, device=DEV)


def _hydro_wrench(eng, cur, old, n, dt=DT):
    """The fp32 hydrodynamic wrench of (cur, previous velocity in old): what the fused kernels integrate (tests/test_closed_loop_gpu.py)."""
    return eng.step_wrench_tiled(cur, n, dt, prev=old)


def _report(label, worst):
    per_group = {g: max(w[g] for w in worst.values()) for g in io.GROUPS}
    print(f"[{label}] max ulps " + "  ".join(f"{g} {v:.2f}" for g, v in per_group.items()) + f"  (bound {B:g})")
    bad = {n: w for n, w in worst.items() if max(w.values()) > B}
    assert not bad, (label, bad)


def _k(comps, st, pr, coeff, n, rho=RHO):
    return io.drag_jacobian(st[:n], pr[:n], {c: comps[c][:n] for c in ("ratio", "area", "scale")}, rho, coeff)


def _push(sc, seed, scale=5.0):
    """(n, 6): forces up to `scale` N per kg, torques up to that times 0.5 m."""
    rng = np.random.default_rng(seed)
    m = sc.params[:, 10:11].astype(np.float64)
    return np.concatenate([rng.uniform(-1, 1, (sc.n, 3)) * scale * m, rng.uniform(-1, 1, (sc.n, 3)) * scale * 0.5 * m], axis=1).astype(np.float32)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- strides and guard regions (C ABI) ------------------------------------------------------------------------------------------------
def _guarded(arr, stride):
    """(n,F) fp32 -> flat device buffer of ceil(n/64) tiles of `stride` floats: field f of body i at
    [(i // 64) * stride + f * 64 + i % 64]; everything else (bodies past n, the stride padding) is NaN."""
    n, f = arr.shape
    tiles = (n + 63) // 64
    flat = np.full((tiles * 64, f), np.nan, np.float32)
    flat[:n] = arr
    host = np.full((tiles, stride), np.nan, np.float32)
    host[:, :f * 64] = flat.reshape(tiles, 64, f).transpose(0, 2, 1).reshape(tiles, f * 64)
    return torch.from_numpy(host.reshape(-1)).to(DEV)


def _unguard(buf, n, fields, stride):
    """-> ((n,F) bodies, the host copy of every float that is NOT a body's field: must still be NaN)."""
    host = buf.cpu().numpy().reshape(-1, stride)
    tiles = host.shape[0]
    flat = host[:, :fields * 64].reshape(tiles, fields, 64).transpose(0, 2, 1).reshape(tiles * 64, fields)
    return flat[:n].copy(), np.concatenate([flat[n:].reshape(-1), host[:, fields * 64:].reshape(-1)])


ARENA_GAP = 8192                                                  # floats between two buffers of an arena: see _in_one_allocation


def _in_one_allocation(*bufs):
    """Flat fp32 device buffers -> views of the same sizes and contents inside ONE allocation, in the order given, ARENA_GAP
    floats of NaN in front of, between and behind them.  For the refusal tests: a call that hands a buffer to the library as
    ANOTHER record makes the library claim that record's extent from the buffer's address - the statistics record's
    (tiles - 1) * stride + 704 floats, 4 404 at six tiles of stride 740, from a `prev` of 2 424 floats - and what lies behind a
    buffer of its own allocation is wherever the allocator put the next one: an output, and the refusal "overlaps an output"
    fires in front of the one the test is about.  Inside the arena a claim of up to ARENA_GAP floats past a buffer's end meets
    only the gap, so every call's only overlap is the intended one, wherever the allocator places the arena."""
    sizes = [b.numel() for b in bufs]
    offsets, at = [], ARENA_GAP
    for size in sizes:
        offsets.append(at)
        at += -(-size // 64) * 64 + ARENA_GAP                       # (every view starts on a 256-byte boundary of the arena)
    arena = torch.full((at,), NAN, dtype=torch.float32, device=DEV)
    views = [arena[o:o + size] for o, size in zip(offsets, sizes)]
    for view, buf in zip(views, bufs):
        assert buf.dtype == torch.float32 and buf.dim() == 1
        view.copy_(buf)
    return views


def _untouched(buf, before):
    """An input buffer, sentinels included, is bit for bit what it was."""
    return np.array_equal(buf.cpu().numpy(), before, equal_nan=True)


def _relative(eng, st, pv, n, step, dt=DT):
    """(s_rel, pv_rel) built on the host in fp32 from hydro_sea_sample's output at `step` steps of `dt`."""
    w = scenes.from_tiled(eng.sea_sample(_tiled(st[:n]), n, step, dt).cpu().numpy(), n)
    return sr.relative(st[:n], pv[:n], w[:, 0], w[:, 1:4])


# ---- one launch through the engine -------------------------------------------------------------------------------------------------------
# entry -> (the HydroEngine method, what it takes between `steps` and `frame`, in its signature's order)
ENTRIES = {
    "app": ("step_fused_tiled_multi_applied", ("applied",)),
    "ctl": ("step_fused_tiled_multi_controlled", ("control", "applied")),
    "sea": ("step_fused_tiled_multi_sea", ("step0", "control", "applied")),
    "bed": ("step_fused_tiled_multi_bed", ("step0", "control", "applied")),
    "moor": ("step_fused_tiled_multi_moor", ("step0", "mooring", "control", "applied")),
    "ext": ("step_fused_tiled_multi_ext", ("step0", "extremes", "mooring", "control", "applied")),
    "teth": ("step_fused_tiled_multi_teth", ("step0", "tether", "extremes", "mooring", "control", "applied")),
    "net": ("step_fused_tiled_multi_net", ("step0", "tether", "layers", "extremes", "mooring", "control", "applied")),
    "peak": ("step_fused_tiled_multi_peak", ("step0", "tether", "layers", "peaks", "extremes", "mooring", "control", "applied")),
    "spread": ("step_fused_tiled_multi_spread", ("step0", "mooring", "mooring_layers", "tether", "layers", "peaks", "extremes", "control", "applied")),
    "irr": ("step_fused_tiled_multi_irr", ("step0", "mooring", "mooring_layers", "tether", "layers", "peaks", "extremes", "control", "applied")),
    "stat": ("step_fused_tiled_multi_stat", ("step0", "statistics", "levels", "channel_a", "channel_b", "mooring", "mooring_layers", "tether", "layers", "peaks",
                                             "extremes", "control", "applied")),
}
COUNTS = {"layers": 1, "mooring_layers": 1, "channel_a": 2, "channel_b": 6}      # what an entry that takes a count is given where the caller names none


def step(eng, entry, cur, old, n, steps, *, step0=0, applied=None, frame="world", control=None, mooring=None, extremes=None, tether=None,
         layers=None, peaks=None, mooring_layers=None, statistics=None, levels=None, channels=None, implicit=False, ke=None, dt=DT, **kw):
    """One launch of `entry` through the engine; returns (state, prev_out): the buffer that received the final state and the six
    velocity fields of the other one.  An option the entry does not take must be None (step0: 0); `layers` is the net's and
    `mooring_layers` the spread's, for the entries that take one (1 where the caller names none); `channels` the statistics' pair
    ((z, tension) likewise).  The sea spectrum is the engine's (set_sea_spectrum), like the sea and the bed.  dt: the step, a Python
    double (the scene's rho and g are the engine's: HydroEngine(n, DEV, rho, g))."""
    method, takes = ENTRIES[entry]
    given = dict(step0=step0, applied=applied, control=control, mooring=mooring, extremes=extremes, tether=tether, layers=layers, peaks=peaks,
                 mooring_layers=mooring_layers, statistics=statistics, levels=levels, channel_a=None if channels is None else channels[0],
                 channel_b=None if channels is None else channels[1])
    for name, value in given.items():
        assert name in takes or value is None or (name == "step0" and value == 0), (entry, name)
        if value is None and name in takes and name in COUNTS and entry in ("spread", "irr", "stat"):
            given[name] = COUNTS[name]
    getattr(eng, method)(cur, old, n, dt, steps, *(given[name] for name in takes), frame, implicit_drag=implicit, ke_out=ke, **kw)
    return old, cur[:, 7:13]


# ---- one call of the C ABI ---------------------------------------------------------------------------------------------------------------
# entry -> what follows `&rows_written` in hydro_step_fused_tiled_multi_<entry>, in its signature's order; a record is followed by
# its tile stride, `applied` by its stride and the frame
RAW_EXTRAS = {
    "app": ("applied",),
    "ctl": ("applied", "control"),
    "sea": ("applied", "control", "step0"),
    "bed": ("applied", "control", "step0"),
    "moor": ("applied", "control", "mooring", "step0"),
    "ext": ("applied", "control", "mooring", "extremes", "step0"),
    "teth": ("applied", "control", "mooring", "extremes", "tether", "step0"),
    "spread": ("applied", "control", "mooring", "mooring_layers", "extremes", "tether", "tether_layers", "peaks", "step0"),
    "irr": ("applied", "control", "mooring", "mooring_layers", "extremes", "tether", "tether_layers", "peaks", "step0"),
    "stat": ("applied", "control", "mooring", "mooring_layers", "extremes", "tether", "tether_layers", "peaks", "statistics", "levels", "channels", "step0"),
}


def raw(eng, entry, n, state, prev, out, pvo, *, steps=1, step0=0, implicit=0, log=None, fields=13, frame=0, applied=None, control=None,
        mooring=None, extremes=None, tether=None, s_applied=S_A, s_control=S_C, s_mooring=S_M, s_extremes=None, s_tether=None,
        mooring_layers=1, tether_layers=1, peaks=None, s_peaks=None, statistics=None, s_statistics=None, levels=None, s_levels=None, channels=(2, 6)):
    """hydro_step_fused_tiled_multi_<entry> with the guard tests' strides on state, prev, out and pvo; records as tensors,
    addresses or None, each with its tile stride (the extremes' and the tether's differ between modules: no default; an absent
    record's stride may be None: 0 is passed).  The counts of "spread", "irr" and "stat" follow their records, the channels the levels.  The
    recorder's arguments are fixed: 8 watched bodies at most, 4 rows, `fields` fields, every 1, phase 1, row0 0.  Returns
    (rc, rows_written); rows_written starts from the sentinel -7."""
    ptr = lambda b: b.data_ptr() if hasattr(b, "data_ptr") else b  # noqa: E731
    records = dict(applied=(applied, s_applied), control=(control, s_control), mooring=(mooring, s_mooring), extremes=(extremes, s_extremes),
                   tether=(tether, s_tether), peaks=(peaks, s_peaks), statistics=(statistics, s_statistics), levels=(levels, s_levels))
    scalars = dict(step0=(step0,), mooring_layers=(mooring_layers,), tether_layers=(tether_layers,), channels=tuple(channels))
    extras = []
    for name in RAW_EXTRAS[entry]:
        if name in scalars:
            extras += scalars[name]
            continue
        record, stride = records.pop(name)
        assert stride is not None or (record is None and entry in ("spread", "irr", "stat")), (entry, name)
        stride = 0 if stride is None else stride
        extras += [ptr(record), stride] + ([frame] if name == "applied" else [])
    assert all(record is None for record, _ in records.values()), (entry, sorted(records))
    written = ctypes.c_int64(-7)
    rc = getattr(eng._lib, f"hydro_step_fused_tiled_multi_{entry}")(
        eng._h, n, ptr(state), S_IN, ptr(prev), S_PV, DT, steps, ptr(out), S_OUT, ptr(pvo), S_PVO,
        int(implicit), 1, None, ptr(log), 8, 4, fields, 1, 1, 0, ctypes.byref(written), *extras, eng._stream(None))
    return rc, written.value


# ---- one step against fp64 -----------------------------------------------------------------------------------------------------------------
def step_wrench_terms(st, hydro, *, applied=None, frame="world", ctl=None, bed_wrench=None, bed_scale=None):
    """(total, surrogate) of one step.  total: the fp64 sum, left to right, of `hydro` (the device's fp32 hydrodynamic wrench),
    `applied` (frame "body": R a | R a), the pose-hold law of `ctl` and `bed_wrench` (any fp64 wrench behind the law: the bed's,
    the lines').  surrogate: what io.field_scales takes in its place, |F_hydro,i| + |f_applied| + |the law's linear terms| +
    bed_scale_i in columns 0 .. 2 and |tau_hydro| + |tau_applied| + the law's angular terms + |bed_scale_tau| in column 3 - a
    thrust that cancels the water does not shrink the yardstick.  An absent term contributes nothing."""
    total = hydro.astype(np.float64)
    surrogate = np.zeros_like(total)
    surrogate[:, 0:3] = np.abs(total[:, 0:3])
    surrogate[:, 3] = np.linalg.norm(total[:, 3:6], axis=1)
    if applied is not None:
        a64 = applied.astype(np.float64)
        if frame == "body":
            R = ho._rot_batch(st[:, 3:7].astype(np.float64))
            a64 = np.concatenate([np.einsum("nab,nb->na", R, a64[:, 0:3]), np.einsum("nab,nb->na", R, a64[:, 3:6])], axis=1)
        total = total + a64
        surrogate[:, 0:3] = surrogate[:, 0:3] + np.linalg.norm(a64[:, 0:3], axis=1, keepdims=True)
        surrogate[:, 3] = surrogate[:, 3] + np.linalg.norm(a64[:, 3:6], axis=1)
    if ctl is not None:
        lin, ang = phr.term_magnitudes(st, ctl)
        total = total + phr.wrench(st, ctl)
        surrogate[:, 0:3] = surrogate[:, 0:3] + np.linalg.norm(lin, axis=1, keepdims=True)
        surrogate[:, 3] = surrogate[:, 3] + ang
    if bed_wrench is not None:
        total = total + bed_wrench
        surrogate[:, 0:3] += bed_scale[:, 0:3]
        surrogate[:, 3] += np.linalg.norm(bed_scale[:, 3:6], axis=1)
    return total, surrogate


def fp64_step_errors(got, st, hydro, pr, k, dt=DT, g=G, **terms):
    """integrator_error_ulps of one step against io.integrate of step_wrench_terms' total, with io.field_scales of its
    surrogate; per field group the largest over the bodies.  `terms`: the keywords of step_wrench_terms.  dt, g: the step and the
    gravity of the launch, as doubles (rho enters through `hydro` and `k`)."""
    total, surrogate = step_wrench_terms(st, hydro, **terms)
    ref = io.integrate(st, total, pr, g, dt, *(k or (None, None)))
    sc = io.field_scales(st, surrogate, pr, g, dt, k, ref)
    err = io.integrator_error_ulps(got, ref, st, total, pr, g, dt, k, scales=sc)
    return {g: float(np.nan_to_num(e, nan=np.inf).max(initial=0.0)) for g, e in err.items()}
