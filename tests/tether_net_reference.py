"""The tether net of hydro_step_fused_tiled_multi_net (include/hydro.h, "Tether net") in fp64: a thin wrapper over
tests/tether_reference.py and tests/closed_loop_reference.py, which stay as they are.  No device, no library, nothing of
silver2_isaacsim_amd.tether.

A net is an (n, 7 L) array, layer l in columns 7 l .. 7 l + 6, each layer a record of tether_reference.  Every line sees the
TRUE state the step starts from; the net's wrench is the sum over the layers.

THE STEP.  closed_loop_reference.closed_loop knows one tether record.  Its step forms hydro + applied + bed + mooring +
tether in fp64 and rounds the sum to fp32 ONCE, so layers 1 .. L - 1 can ride in `applied`: a step of the net is
    closed_loop(..., steps=1, teth=layer 0, applied=applied + sum_{l >= 1} tether_reference.wrench(layer l, state))
and a run is that, chained step by step (the applied wrench depends on the state).  The order of the terms of an fp64 sum
moves it by fp64 dust only.
"""
import numpy as np

import tether_reference as tr
from closed_loop_reference import closed_loop

FIELDS = tr.FIELDS
LAYERS_MAX = 4


def layers_of(net):
    """The (n, 7) records of an (n, 7 L) net."""
    net = np.asarray(net)
    assert net.ndim == 2 and net.shape[1] % FIELDS == 0 and 1 <= net.shape[1] // FIELDS <= LAYERS_MAX, net.shape
    return [net[:, FIELDS * l:FIELDS * (l + 1)] for l in range(net.shape[1] // FIELDS)]


def wrench(net, state, taut=None):
    """(n, 6) the net's W in fp64: the sum over the layers; `taut`: per layer, which lines are stretched (default: decided in fp64)."""
    return sum(tr.wrench(rec, state, None if taut is None else taut[l]) for l, rec in enumerate(layers_of(net)))


def wrench_scales(net, state, taut=None):
    """(n, 6) what an fp32 evaluation of the net's W rounds against: the sum of the layers' tether_reference.wrench_scales."""
    return sum(tr.wrench_scales(rec, state, None if taut is None else taut[l]) for l, rec in enumerate(layers_of(net)))


def tensions(net, state):
    """(L, n) T of each body's line in each layer, fp64."""
    return np.stack([tr.tension(rec, state) for rec in layers_of(net)])


def pulls(net, state):
    """(L, n) bool: the body's line of that layer pulls, by the fp64 reference."""
    return tensions(net, state) > 0


def closed_loop_net(state, prev, params, rho, g, dt, steps, *, net, applied=None, step0=0, **kw):
    """closed_loop_reference.closed_loop with a net: per-step dicts as closed_loop returns them ('tether_*' are layer 0's) with
    'net_tension' (L, n) and 'net_line' (n, 6, the fp64 sum over the layers) added.  `kw`: closed_loop's other keywords."""
    recs = layers_of(net)
    st, pv = np.asarray(state, np.float32), np.asarray(prev, np.float32)
    out = []
    for i in range(steps):
        push = None if applied is None else np.asarray(applied, np.float64)
        for rec in recs[1:]:
            w = tr.wrench(rec, st)
            push = w if push is None else push + w
        r = closed_loop(st, pv, params, rho, g, dt, 1, teth=recs[0], applied=push, step0=step0 + i, **kw)[0]
        r["net_tension"], r["net_line"] = tensions(net, st), wrench(net, st)
        out.append(r)
        pv, st = st[:, 7:13].copy(), r["state"]
    return out
