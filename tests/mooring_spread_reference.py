"""The mooring spread of hydro_step_fused_tiled_multi_spread (include/hydro.h, "Mooring spread") in fp64: a thin wrapper over
tests/mooring_reference.py and tests/closed_loop_reference.py, which stay as they are.  No device, no library, nothing of
silver2_isaacsim_amd.mooring.

A spread is an (n, 9 L) array, layer l in columns 9 l .. 9 l + 8, each layer a record of mooring_reference.  Every line sees the
TRUE state the step starts from; the spread's wrench is the sum over the layers, and the tension the extremes record takes is
the largest over the layers.

THE STEP.  closed_loop_reference.closed_loop knows one mooring record.  Its step forms hydro + applied + bed + mooring + tether
in fp64 and rounds the sum to fp32 ONCE, so layers 1 .. L - 1 can ride in `applied`: a step of the spread is
    closed_loop(..., steps=1, moor=layer 0, applied=applied + sum_{l >= 1} mooring_reference.wrench(layer l, state))
and a run is that, chained step by step (the applied wrench depends on the state).  The order of the terms of an fp64 sum
moves it by fp64 dust only.
"""
import numpy as np

import mooring_reference as mr
from closed_loop_reference import closed_loop

FIELDS = mr.FIELDS
LAYERS_MAX = 4


def layers_of(spread):
    """The (n, 9) records of an (n, 9 L) spread."""
    spread = np.asarray(spread)
    assert spread.ndim == 2 and spread.shape[1] % FIELDS == 0 and 1 <= spread.shape[1] // FIELDS <= LAYERS_MAX, spread.shape
    return [spread[:, FIELDS * l:FIELDS * (l + 1)] for l in range(spread.shape[1] // FIELDS)]


def wrench(spread, state, taut=None):
    """(n, 6) the spread's W in fp64: the sum over the layers; `taut`: per layer, which lines are stretched (default: fp64's decision)."""
    return sum(mr.wrench(rec, state, None if taut is None else taut[l]) for l, rec in enumerate(layers_of(spread)))


def wrench_scales(spread, state, taut=None):
    """(n, 6) what an fp32 evaluation of the spread's W rounds against: the sum of the layers' mooring_reference.wrench_scales."""
    return sum(mr.wrench_scales(rec, state, None if taut is None else taut[l]) for l, rec in enumerate(layers_of(spread)))


def tensions(spread, state):
    """(L, n) T of each body's line in each layer, fp64 (0 where a line adds nothing)."""
    return np.stack([mr.tension(rec, state) for rec in layers_of(spread)])


def pulls(spread, state):
    """(L, n) bool: the body's line of that layer pulls, by the fp64 reference."""
    return tensions(spread, state) > 0


def closed_loop_spread(state, prev, params, rho, g, dt, steps, *, spread, applied=None, step0=0, **kw):
    """closed_loop_reference.closed_loop with a spread: per-step dicts as closed_loop returns them ('line', 'tension', 'taut' are
    layer 0's) with 'spread_tension' (L, n) and 'spread_line' (n, 6, the fp64 sum over the layers) added.  `kw`: closed_loop's
    other keywords."""
    recs = layers_of(spread)
    st, pv = np.asarray(state, np.float32), np.asarray(prev, np.float32)
    out = []
    for i in range(steps):
        push = None if applied is None else np.asarray(applied, np.float64)
        for rec in recs[1:]:
            w = mr.wrench(rec, st)
            push = w if push is None else push + w
        r = closed_loop(st, pv, params, rho, g, dt, 1, moor=recs[0], applied=push, step0=step0 + i, **kw)[0]
        r["spread_tension"], r["spread_line"] = tensions(spread, st), wrench(spread, st)
        out.append(r)
        pv, st = st[:, 7:13].copy(), r["state"]
    return out
