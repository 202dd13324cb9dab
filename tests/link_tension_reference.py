"""The peak tension of every tether link (hydro_step_fused_tiled_multi_peak; include/hydro.h, "Link tensions") in fp64: a thin
wrapper over tests/tether_net_reference.py, which stays as it is.  No device, no library, nothing of silver2_isaacsim_amd.

The record's sample of body i, layer l, in a step is the tension of that line for the state the step STARTS from - what
tether_net_reference.closed_loop_net returns as 'net_tension' - and the record is the running maximum of the samples: the peak of
a run is the fold of 'net_tension' over its steps.
"""
import numpy as np

import tether_net_reference as tnr


def fold(samples):
    """(L, n) running maximum of (steps, L, n) samples from the empty record (+0), with the record's rule M = x if x > M else M (a
    NaN sample never enters), and (L, n) the step whose sample the maximum is (-1: no sample ever entered)."""
    samples = np.asarray(samples, np.float64)
    peak = np.zeros(samples.shape[1:])
    when = np.full(samples.shape[1:], -1)
    with np.errstate(invalid="ignore"):
        for i, x in enumerate(samples):
            enters = x > peak
            peak, when = np.where(enters, x, peak), np.where(enters, i, when)
    return peak, when


def closed_loop_peaks(state, prev, params, rho, g, dt, steps, *, net, **kw):
    """tether_net_reference.closed_loop_net, and the fold of its 'net_tension' over the steps: (peak (L, n) fp64, when (L, n), the
    per-step dicts).  `kw`: closed_loop_net's other keywords."""
    rows = tnr.closed_loop_net(state, prev, params, rho, g, dt, steps, net=net, **kw)
    peak, when = fold(np.stack([r["net_tension"] for r in rows]))
    return peak, when, rows
