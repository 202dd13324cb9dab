"""A sea state for the closed loop: a steady uniform current and up to eight regular deep-water wave components.

`SeaState` is what `ClosedLoopSim.set_sea` and `HydroEngine.set_sea` take.  The kernels evaluate the model of
include/hydro.h ("Sea state") in fp32 inside every physics step; `elevation` and `velocity` below restate it on the host
in fp64 NumPy - for plotting, for choosing a mooring, for checking a recorded trajectory against the surface it rode.

    eta(x, y, t) = sum_j a_j cos(kx_j x + ky_j y - omega_j t + phi_j)
    u(x, y, z_rel, t) = U + sum_j a_j omega_j exp(kappa_j min(z_rel, 0)) (kx_j / kappa_j cos th_j, ky_j / kappa_j cos th_j, sin th_j)

with z_rel the depth of the point below the local surface (z - eta) and kappa_j = |k_j|.  The library takes omega and k
as given; `regular` applies the deep-water dispersion relation omega^2 = g kappa.

`SeaSpectrum` is the same model with up to 64 components - an irregular sea - and `pierson_moskowitz` / `jonswap` build one from
a significant wave height and a peak period (include/hydro.h, "Sea spectrum").

`SeaEnsemble` is several such spectra in one run, each over its own block of the bodies - `jonswap_ensemble` and
`pierson_moskowitz_ensemble` build one sea per seed (include/hydro.h, "Sea ensemble").

A `SeaSpectrum` or `SeaEnsemble` with a `depth` (m) is a FINITE-DEPTH sea: the same surface, the orbital velocity with the profiles
cosh(kappa (z + h)) / sinh(kappa h) and sinh(kappa (z + h)) / sinh(kappa h) in place of exp(kappa z), nothing below the bed
(include/hydro.h, "Finite-depth sea").  `wavenumber` solves omega^2 = g kappa tanh(kappa h), and `depth=` on
the four constructors places the same bins and amplitudes on the shorter waves of that depth.

`CurrentProfile` is a SHEARED current: up to 16 knots (z_l, V_l), piecewise linear over the depth below the instantaneous surface,
added to the water of a finite-depth sea (include/hydro.h, "Current profile").  `power_law` and `slab` are
the two profiles design codes name; `+` superposes them.
"""
from __future__ import annotations

import math

import numpy as np

WAVES_MAX = 8
SPECTRUM_WAVES_MAX = 64
ENSEMBLE_MAX = 1024
CURRENT_KNOTS_MAX = 16


class SeaState:
    _CAP, _KIND = WAVES_MAX, "a sea"

    def __init__(self, current=(0.0, 0.0, 0.0)):
        cur = tuple(float(x) for x in current)
        if len(cur) != 3 or not all(math.isfinite(x) for x in cur):
            raise ValueError("current: expected three finite numbers (m/s, world frame)")
        self.current = cur
        self.waves: list[tuple[float, float, float, float, float]] = []     # (amplitude, kx, ky, omega, phase)

    def add_wave(self, amplitude: float, kx: float, ky: float, omega: float, phase: float = 0.0) -> "SeaState":
        """One regular component: amplitude (m, >= 0), wave vector (kx, ky) (rad/m), angular frequency (rad/s), phase (rad)."""
        w = (float(amplitude), float(kx), float(ky), float(omega), float(phase))
        if not all(math.isfinite(x) for x in w):
            raise ValueError("wave component: non-finite value")
        if w[0] < 0.0:
            raise ValueError("wave component: the amplitude must be >= 0")
        if w[0] != 0.0 and math.hypot(w[1], w[2]) == 0.0:
            raise ValueError("wave component: a wave with amplitude needs a wave vector")
        if len(self.waves) >= self._CAP:
            raise ValueError(f"{self._KIND} has at most {self._CAP} wave components")
        self.waves.append(w)
        return self

    @classmethod
    def regular(cls, height: float, period: float, heading_deg: float, phase: float = 0.0, g: float = 9.81,
                current=(0.0, 0.0, 0.0)) -> "SeaState":
        """One regular deep-water wave of crest-to-trough `height` (m) and `period` (s) travelling towards `heading_deg`
        (degrees from +x towards +y): omega = 2 pi / period, kappa = omega^2 / g."""
        if not period > 0.0 or not g > 0.0:
            raise ValueError("period and g must be > 0")
        omega = 2.0 * math.pi / period
        kappa = omega * omega / g
        h = math.radians(heading_deg)
        return cls(current).add_wave(0.5 * height, kappa * math.cos(h), kappa * math.sin(h), omega, phase)

    def _phases(self, x, y, t):
        x, y, t = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(t, np.float64)
        return [kx * x + ky * y - om * t + ph for _, kx, ky, om, ph in self.waves]

    def elevation(self, x, y, t) -> np.ndarray:
        """Surface elevation eta (m) at (x, y) and time t; the arguments broadcast."""
        x, y, t = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(t, np.float64))
        eta = np.zeros(x.shape, np.float64)
        for (a, *_), th in zip(self.waves, self._phases(x, y, t)):
            eta = eta + a * np.cos(th)
        return eta

    def velocity(self, x, y, z_rel, t) -> np.ndarray:
        """Water velocity (..., 3) (m/s, world frame) at (x, y), `z_rel` below the local surface (negative: submerged; at
        and above the surface the surface value), at time t; the arguments broadcast."""
        x, y, z, t = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z_rel, np.float64),
                                         np.asarray(t, np.float64))
        u = np.empty(x.shape + (3,), np.float64)
        u[...] = self.current
        zc = np.minimum(z, 0.0)
        for (a, kx, ky, om, _), th in zip(self.waves, self._phases(x, y, t)):
            kappa = math.hypot(kx, ky)
            if kappa == 0.0:
                continue
            e = a * om * np.exp(kappa * zc)
            u[..., 0] += e * (kx / kappa) * np.cos(th)
            u[..., 1] += e * (ky / kappa) * np.cos(th)
            u[..., 2] += e * np.sin(th)
        return u


def wavenumber(omega, depth: float, g: float = 9.81):
    """kappa (rad/m) of a linear wave of angular frequency `omega` (rad/s; a number or an array, >= 0) over still water of `depth`
    (m): the root of omega^2 = g kappa tanh(kappa depth).  Newton's iteration on f(x) = x tanh x - omega^2 depth / g in x = kappa
    depth, started from the deep-water root or the shallow-water one, whichever is larger - f is convex and increasing for x > 0
    and both starts lie at or above the root, so the iteration descends monotonically; it stops when x no longer changes."""
    if not (depth > 0.0 and math.isfinite(depth) and g > 0.0):
        raise ValueError("depth must be finite and > 0, g > 0")
    om = np.asarray(omega, np.float64)
    if not (np.isfinite(om).all() and (om >= 0.0).all()):
        raise ValueError("omega must be finite and >= 0")
    c = om * om * (depth / g)
    x = np.maximum(c, np.sqrt(c))
    for _ in range(64):
        th = np.tanh(x)
        slope = th + x * (1.0 - th * th)
        step = np.divide(x * th - c, slope, out=np.zeros_like(x), where=slope > 0.0)
        nxt = x - step
        if np.array_equal(nxt, x):
            break
        x = nxt
    kappa = x / depth
    return float(kappa) if np.ndim(omega) == 0 else kappa


def _depth(depth):
    """None (deep water) or a finite depth > 0 as a float."""
    if depth is None:
        return None
    depth = float(depth)
    if not (depth > 0.0 and math.isfinite(depth)):
        raise ValueError("depth must be None (deep water) or finite and > 0 (m)")
    return depth


class SeaSpectrum(SeaState):
    """An irregular sea: the model of `SeaState` with up to 64 components, what `ClosedLoopSim.set_sea` and
    `HydroEngine.set_sea_spectrum` take for a sea given by its spectrum (hydro_step_fused_tiled_multi_irr; include/hydro.h,
    "Sea spectrum").  `pierson_moskowitz` and `jonswap` below cut a spectrum of significant wave height Hs and peak period Tp
    into equal-energy bins; `add_wave` builds one by hand.  `elevation` and `velocity` are SeaState's, in fp64.
    `depth` (m; None: deep water) makes it a finite-depth sea (hydro_step_fused_tiled_multi_fd; include/hydro.h, "Finite-depth
    sea"): `ClosedLoopSim.set_sea` then takes it through `HydroEngine.set_sea_finite_depth`, `velocity` follows the depth,
    `elevation` is unchanged.  The components are taken as given: `wavenumber` is the dispersion relation of a depth."""
    _CAP, _KIND = SPECTRUM_WAVES_MAX, "a sea spectrum"

    def __init__(self, current=(0.0, 0.0, 0.0), depth=None):
        super().__init__(current)
        self.depth = _depth(depth)

    def velocity(self, x, y, z_rel, t) -> np.ndarray:
        """`SeaState.velocity` in deep water; with a `depth` h the profiles of linear theory - horizontal a omega cosh(kappa (zc +
        h)) / sinh(kappa h), vertical a omega sinh(kappa (zc + h)) / sinh(kappa h), zc = z_rel clamped to -h .. 0 - evaluated as
        (E +- G) / (1 - q), E = exp(kappa zc), G = exp(-kappa (zc + 2 h)), q = exp(-2 kappa h), which neither overflows nor
        cancels in deep water."""
        if self.depth is None:
            return super().velocity(x, y, z_rel, t)
        h = self.depth
        x, y, z, t = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z_rel, np.float64),
                                         np.asarray(t, np.float64))
        u = np.empty(x.shape + (3,), np.float64)
        u[...] = self.current
        zc = np.maximum(np.minimum(z, 0.0), -h)
        for (a, kx, ky, om, _), th in zip(self.waves, self._phases(x, y, t)):
            kappa = math.hypot(kx, ky)
            if kappa == 0.0:
                continue
            e, g_ = np.exp(kappa * zc), np.exp(-kappa * (zc + 2.0 * h))
            scale = a * om / -math.expm1(-2.0 * kappa * h)
            u[..., 0] += scale * (e + g_) * (kx / kappa) * np.cos(th)
            u[..., 1] += scale * (e + g_) * (ky / kappa) * np.cos(th)
            u[..., 2] += scale * (e - g_) * np.sin(th)
        return u

    def hs(self) -> float:
        """The significant wave height 4 sqrt(m0) of the components, m0 = sum a^2 / 2 (m)."""
        return 4.0 * math.sqrt(sum(0.5 * w[0] * w[0] for w in self.waves))

    @classmethod
    def pierson_moskowitz(cls, hs, tp, heading_deg, **kw) -> "SeaSpectrum":
        return pierson_moskowitz(hs, tp, heading_deg, **kw)

    @classmethod
    def jonswap(cls, hs, tp, heading_deg, **kw) -> "SeaSpectrum":
        return jonswap(hs, tp, heading_deg, **kw)


def pm_fraction(omega, omega_p):
    """The Pierson-Moskowitz spectrum's cumulative energy fraction F(omega) = exp(-1.25 (omega_p / omega)^4)."""
    omega = np.asarray(omega, np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        return np.exp(-1.25 * (omega_p / omega) ** 4)


def cos2_cdf(delta):
    """The cumulative distribution of the spreading function (2 / pi) cos^2(delta) on (-pi/2, pi/2)."""
    delta = np.asarray(delta, np.float64)
    return 0.5 + (delta + np.sin(delta) * np.cos(delta)) / math.pi


def cos2_offsets(n: int) -> np.ndarray:
    """The n quantile midpoints of the cos^2 spreading function, ascending: cos2_cdf(delta_j) = (j + 1/2) / n (bisection to the
    last bit of fp64)."""
    target = (np.arange(n) + 0.5) / n
    lo, hi = np.full(n, -0.5 * math.pi), np.full(n, 0.5 * math.pi)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = cos2_cdf(mid) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def jonswap_bin_medians(omega_p: float, gamma: float, n: int, grid: int = 1 << 16) -> np.ndarray:
    """The medians of the n equal-energy bins of the JONSWAP spectrum
        S(omega) ~ omega^-5 exp(-1.25 (omega_p / omega)^4) gamma^exp(-(omega - omega_p)^2 / (2 sigma^2 omega_p^2)),
    sigma = 0.07 up to the peak and 0.09 above it.  The cumulative spectrum is the Pierson-Moskowitz closed form plus the
    integral of the peak enhancement's EXCESS, S_PM (gamma^r - 1), which lives around the peak only: trapezoids on `grid` points,
    uniform in log(omega) over omega_p / 4 .. 32 omega_p (the excess is below 1e-300 outside).  The inverse is linear
    interpolation on that grid.  gamma = 1 has no excess and differs from the closed-form medians by the interpolation alone."""
    w = omega_p * np.exp(np.linspace(math.log(0.25), math.log(32.0), grid))
    sigma = np.where(w <= omega_p, 0.07, 0.09)
    r = np.exp(-((w - omega_p) ** 2) / (2.0 * sigma * sigma * omega_p * omega_p))
    s_pm = 5.0 * omega_p ** 4 * w ** -5.0 * np.exp(-1.25 * (omega_p / w) ** 4)        # dF / d omega
    excess = s_pm * np.expm1(r * math.log(gamma))
    cum = pm_fraction(w, omega_p) + np.concatenate(([0.0], np.cumsum(0.5 * (excess[1:] + excess[:-1]) * np.diff(w))))
    total = 1.0 + (cum[-1] - pm_fraction(w[-1], omega_p))                              # (the tail above the grid is Pierson-Moskowitz's)
    return np.interp((np.arange(n) + 0.5) / n * total, cum, w)


def _from_bins(hs, omegas, heading_deg, seed, spread, current, g, depth=None) -> SeaSpectrum:
    n = len(omegas)
    rng = np.random.default_rng(seed)
    phases = rng.uniform(-math.pi, math.pi, n)
    headings = np.full(n, math.radians(heading_deg))
    if spread == "cos2":
        headings = headings + cos2_offsets(n)[rng.permutation(n)]
    elif spread is not None:
        raise ValueError("spread must be None (long-crested) or 'cos2'")
    a = hs / math.sqrt(8.0 * n)                                   # equal energy per bin: sum a^2 / 2 = hs^2 / 16
    sea = SeaSpectrum(current, depth)
    for om, ph, hd in zip(omegas, phases, headings):
        kappa = om * om / g if sea.depth is None else wavenumber(float(om), sea.depth, g)
        sea.add_wave(a, kappa * math.cos(hd), kappa * math.sin(hd), om, ph)
    return sea


def _check_sea(hs, tp, components, g):
    if not hs >= 0.0 or not tp > 0.0 or not g > 0.0 or not math.isfinite(hs) or not math.isfinite(tp):
        raise ValueError("hs must be >= 0, tp and g > 0")
    if not 1 <= int(components) <= SPECTRUM_WAVES_MAX:
        raise ValueError(f"components must be in 1 .. {SPECTRUM_WAVES_MAX}")


def pierson_moskowitz(hs: float, tp: float, heading_deg: float, *, components: int = SPECTRUM_WAVES_MAX, seed: int = 0, spread=None,
                      current=(0.0, 0.0, 0.0), g: float = 9.81, depth=None) -> SeaSpectrum:
    """A Pierson-Moskowitz sea of significant wave height `hs` (m) and peak period `tp` (s) travelling towards `heading_deg`,
    as `components` deep-water components (kappa = omega^2 / g) of EQUAL ENERGY, in closed form: component j sits at the median
    of bin j of the cumulative energy fraction F, omega_j = omega_p (1.25 / ln(N / (j + 1/2)))^(1/4), with amplitude
    hs / sqrt(8 N).  Phases: numpy.random.default_rng(seed).uniform(-pi, pi, N).  spread="cos2": the headings are
    heading + delta_j, delta_j the quantile midpoints of (2 / pi) cos^2 (`cos2_offsets`), dealt to the components by a
    permutation drawn from the same generator, after the phases.  `depth` (m): the same bins, amplitudes, phases and headings
    on the wavenumbers of that depth (`wavenumber`), and a finite-depth sea (`SeaSpectrum.depth`)."""
    _check_sea(hs, tp, components, g)
    n, omega_p = int(components), 2.0 * math.pi / tp
    omegas = omega_p * (1.25 / np.log(n / (np.arange(n) + 0.5))) ** 0.25
    return _from_bins(hs, omegas, heading_deg, seed, spread, current, g, depth)


def jonswap(hs: float, tp: float, heading_deg: float, *, gamma: float = 3.3, components: int = SPECTRUM_WAVES_MAX, seed: int = 0, spread=None,
            current=(0.0, 0.0, 0.0), g: float = 9.81, depth=None) -> SeaSpectrum:
    """`pierson_moskowitz` for the JONSWAP spectrum of peak enhancement `gamma` (>= 1): the same equal-energy binning, the bin
    medians from the numerically integrated and inverted cumulative spectrum (`jonswap_bin_medians`); the spectrum is scaled
    so that the components carry hs^2 / 16 exactly.  gamma = 1 is the Pierson-Moskowitz sea."""
    _check_sea(hs, tp, components, g)
    if not gamma >= 1.0 or not math.isfinite(gamma):
        raise ValueError("gamma must be >= 1")
    return _from_bins(hs, jonswap_bin_medians(2.0 * math.pi / tp, float(gamma), int(components)), heading_deg, seed, spread, current, g, depth)


class SeaEnsemble:
    """Several seas in one run: `members` are `SeaSpectrum`s of equally many components, and block m of `bodies_per_sea` bodies
    (a multiple of 64) steps through member m - the seeds, headings and currents a design extreme is taken over, in ONE resident
    launch (`ClosedLoopSim.set_sea`, `HydroEngine.set_sea_ensemble`; hydro_step_fused_tiled_multi_ens; include/hydro.h, "Sea
    ensemble").  Lay the bodies out member by member: the same `bodies_per_sea` designs once per member.  Not a `SeaSpectrum`:
    the water depends on the body.  `split` turns any per-body array into (count, bodies_per_sea, ...), so that
    `ens.split(extremes.tension_max())` is seeds x designs, and `mean_of_maxima` / `std_of_maxima` reduce it over the members."""

    def __init__(self, members, bodies_per_sea: int):
        members = list(members)
        if not 1 <= len(members) <= ENSEMBLE_MAX:
            raise ValueError(f"a sea ensemble has 1 .. {ENSEMBLE_MAX} members")
        if not all(isinstance(m, SeaSpectrum) for m in members):
            raise ValueError("the members of a sea ensemble are SeaSpectrum objects")
        if len({len(m.waves) for m in members}) != 1:
            raise ValueError("every member of a sea ensemble must have the same number of wave components")
        if int(bodies_per_sea) != bodies_per_sea or bodies_per_sea < 64 or bodies_per_sea % 64:
            raise ValueError("bodies_per_sea must be a positive multiple of 64")
        if len({m.depth for m in members}) != 1:
            raise ValueError("every member of a sea ensemble must have the same depth (or none)")
        self.members = members
        self.bodies_per_sea = int(bodies_per_sea)

    @property
    def count(self) -> int:
        return len(self.members)

    @property
    def depth(self):
        """The members' common depth (m), or None in deep water: with a depth the ensemble is a finite-depth sea."""
        return self.members[0].depth

    @property
    def waves(self) -> list:
        """Every member's components, one behind the other: empty exactly when every member is current-only."""
        return [w for m in self.members for w in m.waves]

    def sea_of(self, body):
        """The member (index) body `body` steps through; `body` may be an array."""
        return np.asarray(body, np.int64) // self.bodies_per_sea

    def split(self, values) -> np.ndarray:
        """A per-body array (n, ...) as (count, bodies_per_sea, ...): row m holds member m's bodies.  A view where `values` has
        all count * bodies_per_sea bodies; with fewer (the last member's block is partial) the missing bodies are NaN (floats
        only)."""
        v = np.asarray(values)
        full = self.count * self.bodies_per_sea
        if v.shape[0] > full:
            raise ValueError(f"{v.shape[0]} bodies are more than the ensemble's {self.count} x {self.bodies_per_sea}")
        if v.shape[0] < full:
            if not np.issubdtype(v.dtype, np.floating):
                raise ValueError("a partial last member needs a floating-point array (the missing bodies become NaN)")
            v = np.concatenate([v, np.full((full - v.shape[0],) + v.shape[1:], np.nan, v.dtype)])
        return v.reshape((self.count, self.bodies_per_sea) + v.shape[1:])

    def mean_of_maxima(self, values) -> np.ndarray:
        """Per design (position within a member's block), the mean over the members of a per-body maximum (bodies_per_sea, ...)."""
        return self.split(values).mean(axis=0)

    def std_of_maxima(self, values) -> np.ndarray:
        """Per design, the sample standard deviation (ddof = 1; 0 for a single member) over the members."""
        s = self.split(values)
        return s.std(axis=0, ddof=1) if self.count > 1 else np.zeros(s.shape[1:], s.dtype)

    def elevation(self, x, y, t, body) -> np.ndarray:
        """Surface elevation eta (m) at (x, y) and time t of the member that `body` steps through; the arguments broadcast."""
        x, y, t, member = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(t, np.float64), self.sea_of(body))
        eta = np.zeros(x.shape, np.float64)
        for m in np.unique(member):
            at = member == m
            eta[at] = self.members[int(m)].elevation(x[at], y[at], t[at])
        return eta


def _per_member(value, count, scalar):
    """`value` as one value per member: a single one (`scalar(value)` says so) for all, or a sequence of `count`."""
    if scalar(value):
        return [value] * count
    value = list(value)
    if len(value) != count:
        raise ValueError(f"expected one value or one per member ({count}), got {len(value)}")
    return value


def _ensemble(one, hs, tp, heading_deg, seeds, bodies_per_sea, current, kw) -> SeaEnsemble:
    seeds = list(seeds)
    headings = _per_member(heading_deg, len(seeds), lambda v: np.ndim(v) == 0)
    currents = _per_member(current, len(seeds), lambda v: np.ndim(v) == 1)
    return SeaEnsemble([one(hs, tp, float(hd), seed=sd, current=tuple(cu), **kw) for sd, hd, cu in zip(seeds, headings, currents)], bodies_per_sea)


def jonswap_ensemble(hs: float, tp: float, heading_deg, *, seeds=range(16), bodies_per_sea: int, current=(0.0, 0.0, 0.0), **kw) -> SeaEnsemble:
    """One `jonswap` sea per seed: member i is exactly `jonswap(hs, tp, heading, seed=seeds[i], current=current, **kw)`.
    `heading_deg` and `current` may each be one value for every member or a sequence of one per member."""
    return _ensemble(jonswap, hs, tp, heading_deg, seeds, bodies_per_sea, current, kw)


def pierson_moskowitz_ensemble(hs: float, tp: float, heading_deg, *, seeds=range(16), bodies_per_sea: int, current=(0.0, 0.0, 0.0),
                               **kw) -> SeaEnsemble:
    """`jonswap_ensemble` for `pierson_moskowitz`."""
    return _ensemble(pierson_moskowitz, hs, tp, heading_deg, seeds, bodies_per_sea, current, kw)


class CurrentProfile:
    """A current that varies with depth: knots (z_l, V_l) - z_l <= 0 in m below the local surface, strictly ascending, V_l a
    3-vector in m/s, world frame - piecewise linear between the knots, V_0 below the lowest and V_{K-1} above the highest; what
    `ClosedLoopSim.set_current_profile` and `HydroEngine.set_current_profile` take (hydro_step_fused_tiled_multi_shear;
    include/hydro.h, "Current profile").  The knots are kept AS THE ENGINE SEES THEM, rounded to fp32 (`z`, `v`: float64 arrays of
    fp32 values), and must still ascend strictly after that rounding.  It is added to every member's own steady current, and
    takes effect only in a sea that has a depth.  No knots: no current."""

    def __init__(self, z=(), v=()):
        z64, v64 = np.asarray(z, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1, 3)
        if len(z64) != len(v64):
            raise ValueError("a current profile needs one velocity (three numbers) per knot")
        if len(z64) > CURRENT_KNOTS_MAX:
            raise ValueError(f"a current profile has at most {CURRENT_KNOTS_MAX} knots")
        if not (np.isfinite(z64).all() and np.isfinite(v64).all()):
            raise ValueError("current profile: non-finite knot")
        with np.errstate(over="ignore"):
            zf, vf = z64.astype(np.float32), v64.astype(np.float32)
        if not (np.isfinite(zf).all() and np.isfinite(vf).all()):
            raise ValueError("current profile: a knot out of fp32 range")
        if (zf > 0.0).any():
            raise ValueError("current profile: the knots lie at or below the surface (z <= 0)")
        if not (np.diff(zf) > 0.0).all():
            raise ValueError("current profile: z must be strictly ascending (after rounding to fp32)")
        self.z, self.v = zf.astype(np.float64), vf.astype(np.float64)
        inv, d = self.table()[2:]
        if not (np.isfinite(inv).all() and np.isfinite(d).all()):
            raise ValueError("current profile: a segment's 1 / (z_{l+1} - z_l) or V_{l+1} - V_l is out of fp32 range")

    @property
    def knots(self) -> int:
        return len(self.z)

    def velocity(self, z_rel, depth=None) -> np.ndarray:
        """The profile (..., 3) in m/s at `z_rel` below the local surface, in fp64: linear between the knots, constant beyond
        them.  `depth` (m): z_rel is clamped to -depth first, as the kernels do with the sea's depth."""
        z = np.asarray(z_rel, np.float64)
        if depth is not None:
            z = np.maximum(z, -float(depth))
        out = np.zeros(z.shape + (3,), np.float64)
        if self.knots:
            for i in range(3):
                out[..., i] = np.interp(z, self.z, self.v[:, i])
        return out

    def table(self):
        """The constants the kernels read, as fp32 arrays: (V_0 (3,), z_l (K-1,), inv_l = 1 / (z_{l+1} - z_l) (K-1,),
        D_l = V_{l+1} - V_l (K-1, 3)) - the differences formed in fp64 from the fp32 knots and rounded once."""
        if not self.knots:
            return np.zeros(3, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros((0, 3), np.float32)
        with np.errstate(over="ignore", divide="ignore"):
            inv = (1.0 / np.diff(self.z)).astype(np.float32)
            d = np.diff(self.v, axis=0).astype(np.float32)
        return self.v[0].astype(np.float32), self.z[:-1].astype(np.float32), inv, d

    def __add__(self, other: "CurrentProfile") -> "CurrentProfile":
        """The sum of two profiles on the union of their knots (exact: both are linear between neighbouring knots of the union)."""
        if not isinstance(other, CurrentProfile):
            return NotImplemented
        z = np.union1d(self.z, other.z)
        if len(z) > CURRENT_KNOTS_MAX:
            raise ValueError(f"the sum has {len(z)} knots: a current profile has at most {CURRENT_KNOTS_MAX}")
        return CurrentProfile(z, self.velocity(z) + other.velocity(z))

    @classmethod
    def power_law(cls, speed: float, heading_deg: float, depth: float, exponent: float = 1.0 / 7.0, knots: int = CURRENT_KNOTS_MAX) -> "CurrentProfile":
        """The tidal profile of the design codes (DNV-RP-C205 4.1.4): `speed` (m/s, at the surface) times ((z + depth) / depth) **
        exponent, flowing towards `heading_deg` (degrees from +x towards +y), zero at the bed.  The knots sit at
        z_l = -depth (1 - (l / (knots - 1)) ** 4): dense at the bed, where the power law is steep - with 16 knots the piecewise
        linear profile stays within 0.5 % of the surface speed of the closed form above the lowest 1 % of the depth (uniform knots
        miss by 1.5 %)."""
        depth, knots = _depth(depth), int(knots)
        if depth is None or not 2 <= knots <= CURRENT_KNOTS_MAX:
            raise ValueError(f"power_law needs a depth and 2 .. {CURRENT_KNOTS_MAX} knots")
        if not (math.isfinite(speed) and exponent > 0.0 and math.isfinite(exponent)):
            raise ValueError("speed must be finite, exponent finite and > 0")
        frac = (np.arange(knots) / (knots - 1.0)) ** 4                       # (z + depth) / depth at the knots
        hd = math.radians(heading_deg)
        mag = float(speed) * frac ** float(exponent)
        return cls(-depth * (1.0 - frac), np.stack([mag * math.cos(hd), mag * math.sin(hd), np.zeros(knots)], axis=1))

    @classmethod
    def slab(cls, speed: float, heading_deg: float, thickness: float = 50.0) -> "CurrentProfile":
        """The wind-driven profile of the design codes (DNV-RP-C205 4.1.4): `speed` (m/s) at the surface towards `heading_deg`,
        linear to zero at -thickness (m), nothing below."""
        if not (math.isfinite(speed) and thickness > 0.0 and math.isfinite(thickness)):
            raise ValueError("speed must be finite, thickness finite and > 0")
        hd = math.radians(heading_deg)
        return cls([-float(thickness), 0.0], [[0.0, 0.0, 0.0], [speed * math.cos(hd), speed * math.sin(hd), 0.0]])
