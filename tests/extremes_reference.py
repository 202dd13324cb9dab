"""What the extremes tests compare the device's tension_max with: the kernel's own T emulated in fp32 on the host, the scale an
fp32 evaluation of T rounds against, and the bound that follows from the two by the project's rule.

THE TENSION BOUND.  T = max(0, fma(k, x, -(c un))) with x = l - L0: the subtraction cancels, so T rounds against the terms
that form it, not against itself - tension_scale = k (l^ + L0) + c u^, with l^ and u^ the sums of term magnitudes of
mooring_reference.wrench_scales.  Errors of the header's fp32 order emulated on the host (mooring_reference._fp32_terms: a
correctly rounded seed for the reciprocal square root) against mooring_reference.tension (fp64) over the designed population
of tests/test_mooring.py, the eight bodies at the tie aside, in units of 2^-24 of that scale: 0.77 at most.  The rule: the next
power of two at or above twice the largest, 2 x 0.77 = 1.53 -> TENSION_BOUND = 2 (tests/test_extremes.py recomputes it)."""
import numpy as np

import mooring_reference as mr

TENSION_BOUND = 2.0


def tension_fp32_emulated(rec, state):
    """(n,) float32: the T of include/hydro.h's order in NumPy float32, +0 where the line adds nothing."""
    _, _, _, x, T = mr._fp32_terms(rec, state)
    on = mr.has_line(np.asarray(rec, np.float32)) & (x > 0) & (T > 0)
    return np.where(on, T, np.float32(0)).astype(np.float32)


def tension_scale(rec, state):
    """(n,) fp64: k (l^ + L0) + c u^ of mooring_reference.wrench_scales, for every body (meaningful for those with a line)."""
    m, st = np.asarray(rec, np.float64), np.asarray(state, np.float64)
    _, _, l, _, _, _ = mr.geometry(rec, state)
    x, y, z, w = (np.abs(st[:, 3 + i]) for i in range(4))
    Rh = np.empty((len(st), 3, 3))
    Rh[:, 0, 0], Rh[:, 1, 1], Rh[:, 2, 2] = 1 + 2 * (y * y + z * z), 1 + 2 * (x * x + z * z), 1 + 2 * (x * x + y * y)
    Rh[:, 0, 1] = Rh[:, 1, 0] = 2 * (x * y + w * z)
    Rh[:, 0, 2] = Rh[:, 2, 0] = 2 * (x * z + w * y)
    Rh[:, 1, 2] = Rh[:, 2, 1] = 2 * (y * z + w * x)
    rh = np.einsum("nab,nb->na", Rh, np.abs(m[:, 3:6]))
    eh = np.abs(m[:, 0:3]) + np.abs(st[:, 0:3]) + rh
    lh = np.sqrt((eh * eh).sum(axis=1))
    av, ao = np.abs(st[:, 7:10]), np.abs(st[:, 10:13])
    uh = np.stack([av[:, 0] + ao[:, 1] * rh[:, 2] + ao[:, 2] * rh[:, 1],
                   av[:, 1] + ao[:, 2] * rh[:, 0] + ao[:, 0] * rh[:, 2],
                   av[:, 2] + ao[:, 0] * rh[:, 1] + ao[:, 1] * rh[:, 0]], axis=1)
    unh = (uh * eh).sum(axis=1) / np.where(l > 0, l, 1.0)
    return m[:, 7] * (lh + m[:, 6]) + m[:, 8] * unh
