"""The sea spectrum of hydro_step_fused_tiled_multi_irr (include/hydro.h, "Sea spectrum") for tests/test_sea_spectrum.py and
tests/test_sea_spectrum_gpu.py: the designed spectrum, the population that meets its surface, and `water_fp32`, the header's
arithmetic emulated on the host in NumPy fp32 - what fixes SPECTRUM_VIEW_BOUND before a device is asked.

THE EMULATION restates "WATER AT A BODY" statement for statement.  t, x_j, m_j and tau_j are scalars per component: their two
fp64 FMAs are formed exactly (fractions) and rounded once.  An fp32 FMA is float32(float64(a) * float64(b) + float64(c)): the
product of two fp32 values is exact in fp64, the sum is rounded to fp64 and then to fp32 (a double rounding that differs from
the fused one only on ties of the second).  cos, sin and exp2 are NumPy's fp64 functions rounded to fp32 - correctly rounded
but for ties - where the device takes the hardware's v_cos_f32 / v_sin_f32 / v_exp_f32.

THE BOUND.  `view_errors` gives the largest error of an fp32 view against sea_reference.water (fp64), in units of 2^-24 of
sea_reference.view_scales, over the population at steps 0, 1, 7 and 10^6.  For the designed spectrum of 64 components the
emulation gives E = 1.90 (eta 1.12, u 1.90, z_rel 1.03; the figures are printed by tests/test_sea_spectrum.py), so
SPECTRUM_VIEW_BOUND = the next power of two at or above 2 E = 3.80, which is 4.  The factor 2 covers the hardware's seeds: at
8 components they added at most 11 %.  A device reading above the bound is a finding to explain.
"""
import math
from fractions import Fraction

import numpy as np

import sea_reference as sr
from silver2_isaacsim_amd.sea import SeaSpectrum

F32 = np.float32
VIEW_STEPS = (0, 1, 7, 10 ** 6)
SPECTRUM_VIEW_BOUND = 4.0         # units of 2^-24 of sea_reference.view_scales (derived above, on the host)
COMPONENTS = 64


def designed_spectrum(components=COMPONENTS, current=(0.5, -0.2, 0.05), amplitude=0.03):
    """`components` deep-water components of EQUAL amplitude, every one with a wavelength (6 m .. 200 m, geometric), a heading
    (multiples of the golden angle) and a phase of its own: a dropped, repeated or transposed component moves eta and u by an
    amplitude, many bounds.  The first k components of the 64 are the designed spectrum of k."""
    sea = SeaSpectrum(current)
    for j in range(components):
        lam = 6.0 * (200.0 / 6.0) ** (((j * 37) % COMPONENTS) / (COMPONENTS - 1.0))     # (37 is coprime to 64: neighbours differ widely)
        kappa = 2.0 * math.pi / lam
        head = math.radians(137.50776405003785 * j)
        phase = 2.0 * math.pi * ((0.6180339887498949 * (j + 1)) % 1.0) - math.pi
        sea.add_wave(amplitude, kappa * math.cos(head), kappa * math.sin(head), math.sqrt(9.81 * kappa), phase)
    return sea


def truncated(sea, count):
    """The first `count` components of `sea`, same current."""
    out = SeaSpectrum(sea.current)
    for w in sea.waves[:count]:
        out.add_wave(*w)
    return out


def without(sea, j):
    out = SeaSpectrum(sea.current)
    for i, w in enumerate(sea.waves):
        if i != j:
            out.add_wave(*w)
    return out


def spectrum_population(st, sea):
    """`st` with every body moved up or down by `sea`'s elevation above it at t = 0: the partial ones straddle the DISPLACED surface."""
    st = st.copy()
    st[:, 2] = (st[:, 2].astype(np.float64) + sea.elevation(st[:, 0], st[:, 1], 0.0)).astype(np.float32)
    return st


def _fma64(a, b, c):
    """fma(a, b, c) of three doubles, rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fmaf(a, b, c):
    """fmaf of fp32 values (see the module's docstring)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def water_fp32(sea, px, py, pz, step, dt):
    """(eta (n,) fp32, u (n, 3) fp32): include/hydro.h's order of operations in NumPy fp32 (see the module's docstring)."""
    px, py, pz = (np.asarray(a, F32) for a in (px, py, pz))
    t = float(int(step)) * float(dt)
    inv2pi32 = F32(0.15915494309189535)
    rows = []
    eta = np.zeros(px.shape, F32)
    for a, kx, ky, om, ph in sr._waves(sea):
        kappa = math.sqrt(kx * kx + ky * ky)
        if not kappa > 0.0:                                      # (a == 0: the record is all zeros)
            a = kx = ky = om = ph = 0.0
        x = _fma64(-om, t, ph)
        m = float(np.rint(x * 0.15915494309189535))
        tau = F32(_fma64(-m, 2.4492935982947064e-16, _fma64(-m, 6.283185307179586, x)))
        th = _fmaf(F32(kx), px, _fmaf(F32(ky), py, np.full(px.shape, tau, F32)))
        rev = th * inv2pi32
        r = (rev - np.rint(rev)).astype(np.float64)
        c, s = np.cos(2.0 * math.pi * r).astype(F32), np.sin(2.0 * math.pi * r).astype(F32)
        eta = _fmaf(F32(a), c, eta)
        aw = a * om
        rows.append((c, s, F32(kappa * 1.4426950408889634), F32(aw * kx / kappa) if kappa > 0.0 else F32(0.0),
                     F32(aw * ky / kappa) if kappa > 0.0 else F32(0.0), F32(aw)))
    zc = np.minimum(pz - eta, F32(0.0))
    u = [np.full(px.shape, F32(float(x) + 0.0), F32) for x in sea.current]
    for c, s, kl2, cx, cy, aw in rows:
        e = np.exp2((kl2 * zc).astype(np.float64)).astype(F32)
        ec, es = e * c, e * s
        u[0], u[1], u[2] = _fmaf(cx, ec, u[0]), _fmaf(cy, ec, u[1]), _fmaf(aw, es, u[2])
    return eta, np.stack(u, axis=-1)


def view_errors(sea, st, step, dt, eta32, u32):
    """{eta, u, z_rel}: the largest error of the fp32 view (eta32, u32) of the bodies `st` at `step` against sea_reference.water,
    in units of 2^-24 of sea_reference.view_scales."""
    px, py, pz = st[:, 0], st[:, 1], st[:, 2]
    eta, u = sr.water(sea, px, py, pz, step, dt)
    s_eta, s_u, s_z = sr.view_scales(sea, px, py, pz)
    z_rel = (pz - np.asarray(eta32, F32)).astype(np.float64)                        # the fp32 subtraction the kernel makes
    return {"eta": float((np.abs(eta32 - eta) / (sr.ULP * s_eta)).max()),
            "u": float((np.abs(u32 - u) / (sr.ULP * s_u)).max()),
            "z_rel": float((np.abs(z_rel - (pz.astype(np.float64) - eta)) / (sr.ULP * s_z)).max())}
