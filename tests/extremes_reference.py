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
from rigid_reference import point_velocity_scale, rot_magnitudes

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
    rh = np.einsum("nab,nb->na", rot_magnitudes(st[:, 3:7]), np.abs(m[:, 3:6]))
    eh = np.abs(m[:, 0:3]) + np.abs(st[:, 0:3]) + rh
    lh = np.sqrt((eh * eh).sum(axis=1))
    uh = point_velocity_scale(st[:, 7:10], st[:, 10:13], rh)
    unh = (uh * eh).sum(axis=1) / np.where(l > 0, l, 1.0)
    return m[:, 7] * (lh + m[:, 6]) + m[:, 8] * unh
