"""The sea state of hydro_step_fused_tiled_multi_sea (include/hydro.h, "Sea state") restated in fp64 NumPy: the reference of
tests/test_sea.py and tests/test_sea_gpu.py.  No device, no library, nothing of silver2_isaacsim_amd.sea.

A sea is anything with `current` (3 numbers) and `waves` (rows of amplitude, kx, ky, omega, phase):

    t      = step * dt
    th_j   = kx_j px + ky_j py - omega_j t + phi_j
    eta    = sum_j a_j cos th_j                               z_rel = pz - eta
    u      = U + sum_j a_j omega_j exp(kappa_j min(z_rel, 0)) (kx_j / kappa_j cos th_j, ky_j / kappa_j cos th_j, sin th_j)

The step's wrench is that of the state with s[2] = z_rel, s[7:10] = v - u and of the previous velocity with pv[0:3] - u;
everything behind the wrench takes the true state.
"""
import numpy as np

ULP = 2.0 ** -24
VIEW_BOUND = 4.0              # units of 2^-24 of view_scales: the bound of hydro_sea_sample (tests/test_sea_gpu.py's docstring derives it)


def _waves(sea):
    return [tuple(float(x) for x in w) for w in sea.waves]


def water(sea, px, py, pz, step, dt):
    """(eta (n,), u (n, 3)) in fp64 for bodies at (px, py, pz) at the start of step `step` (an integer, or (n,) of them)."""
    px, py, pz = (np.asarray(a, np.float64) for a in (px, py, pz))
    t = np.asarray(step, np.float64) * float(dt)
    eta = np.zeros(np.broadcast(px, t).shape, np.float64)
    th = []
    for a, kx, ky, om, ph in _waves(sea):
        th.append(kx * px + ky * py - om * t + ph)
        eta = eta + a * np.cos(th[-1])
    zc = np.minimum(pz - eta, 0.0)
    u = np.empty(eta.shape + (3,), np.float64)
    u[...] = np.asarray(sea.current, np.float64)
    for (a, kx, ky, om, _), thj in zip(_waves(sea), th):
        kappa = np.hypot(kx, ky)
        if kappa == 0.0:
            continue
        e = a * om * np.exp(kappa * zc)
        u[..., 0] += e * kx / kappa * np.cos(thj)
        u[..., 1] += e * ky / kappa * np.cos(thj)
        u[..., 2] += e * np.sin(thj)
    return eta, u


def view_scales(sea, px, py, pz):
    """What an fp32 evaluation of the view rounds against, per body: (eta, u (n, 3), z_rel).  Every phase th_j carries the
    rounding of its terms, |kx px| + |ky py| + |tau| with |tau| <= pi counted as 1 in units of the amplitude it multiplies:
        eta   : sum_j a_j (1 + |kx_j px| + |ky_j py|)
        u_i   : |U_i| + sum_j a_j omega_j (1 + |kx_j px| + |ky_j py|)
        z_rel : |pz| + the scale of eta"""
    px, py, pz = (np.asarray(a, np.float64) for a in (px, py, pz))
    s_eta = np.zeros(px.shape, np.float64)
    s_u = np.zeros(px.shape, np.float64)
    for a, kx, ky, om, _ in _waves(sea):
        grow = 1.0 + np.abs(kx * px) + np.abs(ky * py)
        s_eta = s_eta + a * grow
        s_u = s_u + a * abs(om) * grow
    return s_eta, np.abs(np.asarray(sea.current, np.float64))[None, :] + s_u[:, None], np.abs(pz) + s_eta


def relative(state, prev, eta, u):
    """(s_rel, pv_rel) in fp32 from fp32 eta (n,) and u (n, 3): the subtractions the kernel makes, rounded as it rounds them."""
    s, pv = np.array(state, np.float32), np.array(prev, np.float32)
    eta, u = np.asarray(eta, np.float32), np.asarray(u, np.float32)
    s[:, 2] = s[:, 2] - eta
    s[:, 7:10] = s[:, 7:10] - u
    pv[:, 0:3] = pv[:, 0:3] - u
    return s, pv
