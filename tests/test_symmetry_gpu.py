"""Exact sign symmetry of every device entry under mirror_y, mirror_x and the half turn about z (tests/symmetry.py states the
maps and the predicate; DESIGN.md, "Sign symmetry"; the CPU half is tests/test_symmetry.py).

Each test runs an entry on a population and on its image and demands that the image's outputs are the images of the outputs,
by float equality - state, prev_out, wrench, components, ratio, every recorded row, the extremes record (min and max of a
flipped axis swapped) - and that scalars (energy pair, eta, tension) keep their bits.  No tolerance: the maps change signs
only, and a kernel in which every term of every sum has the same parity cannot tell a scene from its image.  The references
of the other GPU tests were written from the same reading of the model as the kernels; this one was written by neither.

THE ONE EXCEPTION is the bed: seabed_wrench accumulates the corners i = 0 .. 7 in index order and the maps permute them
(mirror_y i <-> i ^ 2, mirror_x i <-> i ^ 1, half turn i <-> i ^ 3), so with two or more contributing corners the fp32 sums
run in another order - a sum of more than two terms whose order the map permutes, not a term of the wrong hand.  A body is
ORDER-SENSITIVE from the first step whose input state has two or more contributing corners by seabed_reference (decided in
fp64 or as the kernel decides, whichever counts more; on the recorded states of either run - the reference decides, not the
kernel under test).  Before that step its rows are compared exactly; from it on they are left out and must be finite; the
probe's wrench of such a body is held to 2 x PROBE_BOUND of tests/test_seabed_gpu.py in that test's metric and its one-step
result to 2 x integrator_oracle.STEP_ULP_BOUND in the metric of tests/test_integrator_gpu.py (each run is within one bound
of fp64, and fp64 is symmetric to 1e-12: tests/test_symmetry.py).

THE RESIDENT POPULATIONS.  `designed` is the mooring tests' population (the bed population with line_population's unmoored,
all-taut and mixed tiles).  A quarter of it and more stands on four to eight corners by design (test_population_meets_the_bed),
so more than 25 % of it is order-sensitive from the first step; `reseated` is the same population with most of those bodies
moved, in z only, onto ONE corner and the lines drawn anew for the moved bodies: on it the share left out after 7 steps is
asserted to be at most 25 %.  Both are run; the tests print, per entry, the bodies compared exactly and the bodies left out.
EXPLICIT DRAG.  The population's |k| dt / m reaches 50, far beyond the explicit form's stability: in the fp64 closed loop 249
of the 321 bodies have left the fp32 range after seven explicit steps (tests/test_step_variants_gpu.py: "seven explicit steps
may carry a light body out of range"), and a body on its way out counts eight corners far below the plane.  With explicit drag
the comparisons are the same (a NaN equals a NaN), but "finite" and the 25 % share are asserted under implicit drag only; the
explicit share is printed.

Sizes: n = 200 (one block: three full tiles and 8 lanes) and n = 321 (two blocks, the last wave with one live lane); the
wrench entries: 81, 4 096 and 4 097 bodies.  One engine per population, size and coefficient format, switched with
set_semantics / set_sea / set_seabed / set_tuning / set_watch.

ON AN MI355X (f32 and f16 coefficients, both semantics, explicit and implicit drag alike unless said):
  wrench entries        edge_cases 81 (72 wet), ties 4 096 (2 923 wet), config 4 4 097 (3 060 wet) bodies x 3 maps x 8 entries
                        (ext, tiled, tiled + ke, aos wxyz, aos xyzw, batch, components, components_aos): 0 bodies differ; the
                        energy pair keeps its bits
  integrator, fused     321 bodies x 3 maps x 6 entries (4 with implicit drag): 0 differ; the wrong hand is told apart
  probes                hydro_sea_sample at steps 0 and 10^6 and hydro_mooring_wrench: 0 differ
  hydro_seabed_wrench   1 356 bodies x maps with at most one corner: 0 differ; 207 with two or more: largest difference 1.82
                        units of 2^-24 of the scale (bound 2 x 4)
  resident policies     rec, app (world, body), ctl, ctl + app, sea, all-far: every body exact at 1 and 7 steps, n = 200 and 321.
                        bed, moor, ext, all on `reseated`: 175 / 277 exact and 25 / 44 left out (12 % / 14 %) after one step,
                        the one step of those left out within 7.67 ulps of its image (bound 2 x 24); after 7 implicit steps
                        32 .. 43 of 200 (16 .. 22 %) and 59 .. 72 of 321 (18 .. 22 %) left out, after 7 explicit steps 36 .. 39 %;
                        on `designed` 57 .. 60 % are left out from the first step.  Not one body the reference calls
                        order-insensitive differs in any row.
  everything on         with non_temporal = 1 and under Warp semantics: as above (69 .. 72 of 321 left out after 7 implicit steps)
  ClosedLoopSim         64 moored buoys and their mirror_y image, 20 steps in chunks of 7: 0 bodies differ
  later probes          hydro_tether_wrench (wrench and tension, both layers of the net; 28 % / 26 % of 200 and 29 % / 27 % of 321
                        bodies pulled), hydro_mooring_wrench on each of the spread's four layers (37 % / 44 % / 7 % / none of 200,
                        36 % / 46 % / 4 % / none of 321) and hydro_sea_spectrum_sample at 11 and 64 components, steps 0 and 10^6:
                        0 differ
  later rungs           teth, net, peak, spread, irr, everything on, on tests/symmetry_population.py.  Over FAR at 1 and 7 steps:
                        200 / 321 exact, none left out, under implicit drag and after one explicit step - log, state, prev_out,
                        extremes, link tensions and the energy pair; after 7 explicit steps 7 .. 14 of 200 and 8 .. 19 of 321 have
                        been thrown through FAR's plane and are left out (test_later_rungs_are_exactly_symmetric), the others
                        exact.  Over BED, one step: 175 / 277 exact, 25 / 44 left out (12 % / 14 %), every entry, either drag,
                        f32 and f16.  0 bodies differ.
  irr variants          non_temporal = 1 and Warp semantics, FAR, 7 steps, n = 321: 321 exact under implicit drag (explicit:
                        302 / 303 exact, 19 / 18 thrown through FAR's plane)
  teeth on the device   the net's fairleads turned like axial vectors: 48 .. 58 % of the bodies differ from the predicted image
                        after one step; the spectrum's ky not flipped under mirror_y: 100 %
  top probes            hydro_sea_ensemble_sample (tiles_per_sea 1 and 4), hydro_sea_finite_depth_sample (an ensemble of one, an
                        ensemble) and hydro_current_profile_sample (no profile, 2 and 16 knots), 11 and 64 components, steps 0
                        and 10^6, on 200 and 321 bodies in 3 m of water, sea_depth_reference.population() (130 bodies over the
                        column of 9 m) and a body in every knot interval: 324 images, 0 differ, eta the same bits
  top rungs             stat, ens (tiles_per_sea 1 and 4), fd (an ensemble of one, an ensemble), shear (16 knots, 2 knots), each with
                        everything on and a statistics record over (z, tension) and over (x, vy).  Over FAR at 1 and 7 steps:
                        200 / 321 exact, none left out, under implicit drag and after one explicit step - log, state, prev_out,
                        extremes, link tensions, the record (the up-crossing word of a flipped slot left out) and the energy
                        pair; after 7 explicit steps 10 .. 17 of 200 and 18 .. 21 of 321 thrown through FAR's plane and left out.
                        Over BED, one step: 175 / 277 exact, 25 / 44 left out (12 % / 14 %), every case, either drag, f32 and
                        f16.  0 bodies differ.
  shear variants        non_temporal = 1 and Warp semantics, FAR, 7 steps, n = 321: 321 exact under implicit drag (explicit:
                        300 / 302 exact, 21 / 19 thrown through FAR's plane)
  open-loop sea entries hydro_step_wrench_tiled_sea / _aos_sea under the 8-wave sea, _tiled_irr / _aos_irr under the spectrum, an
                        ensemble and a finite-depth ensemble, both quaternion orders, with the samples at a time, times 0, 7 dt
                        and 10^6 dt: edge_cases 81 bodies (68 wet; 79 under the ensembles), tests/symmetry_population.py 321
                        (all wet) x 3 maps: 0 differ in the wrench, the engine-owned previous velocity or the sample
  top teeth             one implicit step over FAR, n = 200 and 321: the finite-depth sea's ky not flipped under mirror_y 100 %
                        of the bodies differ; the profile's V_l turned like an axial vector (mirror_y, mirror_x) 100 %; ONE
                        member of the ensemble left unturned 100 % of that member's 64 bodies and not one body of another member
  ClosedLoopSim, top    64 moored buoys in a depth-carrying ensemble under the 16-knot profile and their mirror_y image, 20
                        steps in chunks of 7: 0 bodies differ
So every device entry is exactly sign-symmetric under all three maps, but for the bed's corner sum - an order asymmetry, not
a term of the wrong hand: no body with fewer than two contributing corners ever differs.  (The statistics record's up-crossing
word of a flipped channel is no exception to that: the image counts the scene's DOWN-crossings, tests/symmetry.py.)"""
import numpy as np
import pytest
import torch

import current_profile_reference as cpr
import populations
import sea_depth_reference as sdr
import sea_ensemble_harness as seh
import sea_reference as sr
import sea_spectrum_reference as ssr
import seabed_reference as br
import symmetry as sym
import symmetry_population
from conftest import load_golden
from oracle import hydro_oracle as ho
from oracle import integrator_oracle as io
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import scenes
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.engine import HydroEngine
from silver2_isaacsim_amd.mooring import Mooring
from silver2_isaacsim_amd.sea import SeaEnsemble, SeaState
from silver2_isaacsim_amd.simulate import ClosedLoopSim
from designed_populations import BED, bed_pop, contributing_corners, FAR, hold_pop, SEA, tilted_boxes  # noqa: F401  (fixtures are requested by name)
from mooring_population import _buoys, DEPTH, line_population, moored_pop as pop  # noqa: F401  (fixtures are requested by name)
from resident_harness import _buffers, COEFFS, DEV, DRAG, DT, _from, G, _ke, NAN, RHO, _tiled
from seabed_reference import PROBE_BOUND
from tether_net_population import net_for

pytestmark = pytest.mark.gpu
SIZES = (200, 321)
STEPS = (1, 7)
SEMANTICS = ("numba", "warp")
STEP0 = 11
FULL = ssr.designed_spectrum()                                    # 64 components, U = (0.5, -0.2, 0.05)
TWO_WAVES = SeaState((0.5, -0.2, 0.05)).add_wave(*SEA.waves[0]).add_wave(*SEA.waves[1])


@pytest.fixture(scope="module")
def engines(native_built):
    """engines(key, params, coeff, rho, g, copy=0): the module's engine for that population and coefficient format, back at
    its defaults (`copy`: a second engine over the same bodies, for the batched launch)."""
    made = {}

    def get(key, params, coeff, rho=RHO, g=G, copy=0):
        k = (key, len(params), coeff, copy)
        if k not in made:
            made[k] = HydroEngine(len(params), DEV, rho, g)
            made[k].set_params(params, coeff)
        eng = made[k]
        eng.set_tuning()
        eng.set_semantics("numba")
        _no_water(eng)
        eng.set_seabed(None)
        eng.set_watch(None)
        return eng
    yield get
    for eng in made.values():
        eng.close()


def _no_water(eng):
    """Clear the profile and every kind of sea (they exclude each other: one must go before another is set)."""
    eng.set_current_profile(None)
    eng.set_sea_finite_depth(None)
    eng.set_sea_ensemble(None)
    eng.set_sea_spectrum(None)
    eng.set_sea(None)


def _soa(x):
    return torch.from_numpy(scenes.to_soa(np.ascontiguousarray(x, np.float32))).to(DEV)


def _rows(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _np(t):
    return t.cpu().numpy()


# ---- (a) the wrench entries ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrench_pops():
    """name -> (state, prev, params, rho, g, dt): every body of edge_cases (81) and ties (4 096), and config 4 drawn to 4 097
    bodies (65 tiles: more than one block, the last wave with one live lane)."""
    out = {}
    for name in ("edge_cases", "ties"):
        fx = load_golden(name)
        out[name] = tuple(np.ascontiguousarray(fx[k], np.float32) for k in ("state", "prev", "params")) + (float(fx["rho"]), float(fx["g"]), float(fx["dt"]))
    sc = scenes.scene_c4(n=4097, seed=4)
    out["c4"] = (sc.state, sc.prev, sc.params, sc.rho, sc.g, sc.dt)
    return out


def _wrench_entries(eng, other, st, pv, dt):
    """Every wrench entry on (st, pv): name -> (n, 6) wrench, (n, 8, 3) components, (n,) ratio or the energy pair.  `other`:
    a second engine over the same bodies, which takes the second scene of the batched launch - given (st, pv) as well, so
    that the launch holds the scene twice; the caller builds the launch of a scene and its image itself."""
    n = len(st)
    out = {}
    out["ext"] = _np(eng.step_wrench(_soa(st), dt, prev=_soa(pv))).T
    S, P = _tiled(st), _tiled(pv)
    out["tiled"] = _from(eng.step_wrench_tiled(S, n, dt, prev=P), n)
    ke = _ke()
    out["tiled_ke"] = _from(eng.step_wrench_tiled(S, n, dt, prev=P, ke_out=ke), n)
    out["ke"] = _np(ke)
    pos, vel = _rows(st[:, 0:3]), _rows(st[:, 7:13])
    for name, quat, xyzw in (("aos_wxyz", st[:, [6, 3, 4, 5]], False), ("aos_xyzw", st[:, 3:7], True)):
        eng.set_prev_velocity(_soa(pv))
        f, t = eng.step_wrench_aos(pos, _rows(quat), vel, dt, quat_xyzw=xyzw)
        out[name] = np.concatenate([_np(f), _np(t)], axis=1)
    with np.errstate(all="ignore"):
        accel = ((st[:, 7:13].astype(np.float64) - pv.astype(np.float64)) / dt).astype(np.float32)
    comps, ratio = eng.step_components(_soa(st), _soa(accel))
    out["components"], out["ratio"] = _np(comps).T.reshape(n, 8, 3), _np(ratio)
    aos = torch.full((8, n, 3), NAN, dtype=torch.float32, device=DEV)
    r2 = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    eng.step_components_aos(pos, _rows(st[:, 3:7]), _rows(st[:, 7:10]), _rows(st[:, 10:13]), _rows(accel[:, 0:3]), _rows(accel[:, 3:6]), aos, r2)
    out["components_aos"], out["ratio_aos"] = _np(aos).transpose(1, 0, 2), _np(r2)
    torch.cuda.synchronize()
    return out, accel


WRENCHES = ("ext", "tiled", "tiled_ke", "aos_wxyz", "aos_xyzw")


@COEFFS
@pytest.mark.parametrize("semantics", SEMANTICS)
def test_wrench_entries_are_exactly_symmetric(coeff, semantics, wrench_pops, engines):
    """hydro_step_wrench_ext, _tiled (with and without ke_out: the energy pair keeps its bits), _aos in both quaternion orders,
    _tiled_batch with a scene and its image in ONE launch, hydro_step_components and _components_aos: 0 bodies differ."""
    for name, (st, pv, pr, rho, g, dt) in wrench_pops.items():
        n = len(st)
        eng, other = engines(name, pr, coeff, rho, g), engines(name, pr, coeff, rho, g, copy=1)
        eng.set_semantics(semantics)
        other.set_semantics(semantics)
        want, _ = _wrench_entries(eng, other, st, pv, dt)
        wet = want["ratio"] > 0
        assert name == "edge_cases" or (wet.mean() > 0.5 and np.isfinite(want["ext"]).all())
        for m in sym.MAPS:
            st_g, pv_g = sym.state(m, st), sym.prev(m, pv)
            got, _ = _wrench_entries(eng, other, st_g, pv_g, dt)
            for w in WRENCHES:
                bad = sym.differing(got[w], sym.wrench(m, want[w]))
                assert not bad.any(), (name, m, w, int(bad.sum()), np.nonzero(bad)[0][:8])
            assert sym.equal(got["ke"], want["ke"]), (name, m, got["ke"], want["ke"])
            for c, r in (("components", "ratio"), ("components_aos", "ratio_aos")):
                bad = sym.differing(got[c], sym.components(m, want[c])) | sym.differing(got[r], want[r])
                assert not bad.any(), (name, m, c, int(bad.sum()), np.nonzero(bad)[0][:8])
            # the batched launch: the scene and its image side by side
            both = HydroEngine.step_wrench_tiled_batch([eng, other], [_tiled(st), _tiled(st_g)], dt, prevs=[_tiled(pv), _tiled(pv_g)], ns=[n, n])
            torch.cuda.synchronize()
            a, b = _from(both[0], n), _from(both[1], n)
            assert sym.equal(a, want["tiled"]) and not sym.differing(b, sym.wrench(m, a)).any(), (name, m, "batch")
        print(f"[wrench entries {coeff} {semantics}] {name}: {n} bodies ({int(wet.sum())} wet) x 3 maps x 8 entries: 0 differ")


# ---- (b) the integrator and the plain fused steps ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_pop():
    st, pv, pr = populations.integrator_population(n=321, seed=31)
    p16 = pr.copy()
    p16[:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    return st, pv, {"f32": pr, "f16": p16}


def _plain(eng, st, pv, w6, n, implicit):
    """name -> outputs of hydro_integrate, hydro_integrate_tiled (explicit only: they take a wrench), hydro_step_fused_tiled
    without and with ke_out, and hydro_step_fused_tiled_multi at 1 and 7 steps."""
    out = {}
    if not implicit:
        out["integrate"] = (_np(eng.integrate(_soa(st), _soa(w6), DT)).T,)
        out["integrate_tiled"] = (_from(eng.integrate_tiled(_tiled(st), _tiled(w6), n, DT), n),)
    for with_ke in (False, True):
        cur, old = _buffers(st, pv, n)
        ke, wr = (_ke() if with_ke else None), eng.alloc_tiled(6, n)
        new = eng.step_fused_tiled(cur, old, n, DT, wrench=wr, implicit_drag=implicit, ke_out=ke)
        out["fused" + ("_ke" if with_ke else "")] = (_from(new, n), _from(wr, n)) + ((_np(ke),) if with_ke else ())
    for steps in STEPS:
        cur, old = _buffers(st, pv, n)
        ke = _ke()
        new = eng.step_fused_tiled_multi(cur, old, n, DT, steps, implicit_drag=implicit, ke_out=ke)
        out[f"multi{steps}"] = (_from(new, n), _from(cur, n)[:, 7:13], _np(ke))
    torch.cuda.synchronize()
    return out


@COEFFS
@DRAG
@pytest.mark.parametrize("semantics", SEMANTICS)
def test_integrator_and_fused_steps_are_exactly_symmetric(coeff, implicit, semantics, int_pop, engines):
    """n = 321: state out, the wrench hydro_step_fused_tiled hands out, prev_out and the energy pair."""
    st, pv, params = int_pop
    n = len(st)
    eng = engines("integrator", params[coeff], coeff)
    eng.set_semantics(semantics)
    w6 = _from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv)), n)
    want = _plain(eng, st, pv, w6, n, implicit)
    assert np.isfinite(want["multi1"][0]).all() and not sym.equal(want["multi1"][0], st)
    for m in sym.MAPS:
        got = _plain(eng, sym.state(m, st), sym.prev(m, pv), sym.wrench(m, w6), n, implicit)
        for name, outs in want.items():
            image = [sym.state(m, outs[0])]
            if name.startswith("fused"):
                image.append(sym.wrench(m, outs[1]))
            elif name.startswith("multi"):
                image.append(sym.prev(m, outs[1]))
            image += list(outs[len(image):])                         # the energy pair: unchanged
            assert len(image) == len(got[name])
            for k, (a, b) in enumerate(zip(got[name], image)):
                bad = sym.differing(a, b) if a.ndim == 2 else np.array([not sym.equal(a, b)])
                assert not bad.any(), (m, name, k, int(bad.sum()), np.nonzero(bad)[0][:8], a if a.ndim == 1 else None, b if a.ndim == 1 else None)
    # teeth on the device: the image with an angular velocity of the wrong hand (under the half turn: left unturned) is told apart
    spinning = (st[:, 10:13] != 0).any(axis=1)
    for m in sym.MAPS:
        wrong, wrong_pv = sym.state(m, st), sym.prev(m, pv)
        hand = sym.POLAR[m] if m != "half_turn" else sym.SAME3
        wrong[:, 10:13], wrong_pv[:, 3:6] = sym._times(st[:, 10:13], hand), sym._times(pv[:, 3:6], hand)
        cur, old = _buffers(wrong, wrong_pv, n)
        new = _from(eng.step_fused_tiled_multi(cur, old, n, DT, 1, implicit_drag=implicit), n)
        assert sym.differing(new, sym.state(m, want["multi1"][0]))[spinning].mean() >= 0.9, m
    print(f"[integrator and fused steps {coeff} {semantics} {'implicit' if implicit else 'explicit'}] {n} bodies x 3 maps x {len(want)} entries: 0 differ")


# ---- (c) the probes ---------------------------------------------------------------------------------------------------------------------
@COEFFS
def test_sea_sample_and_mooring_probe_are_exactly_symmetric(coeff, pop, engines):
    st, _, params, _, _, rec = pop
    for n in SIZES:
        eng = engines("designed", params[coeff][:n], coeff)
        s, m9 = st[:n], rec[:n]
        for m in sym.MAPS:
            s_g = sym.state(m, s)
            for step in (0, 10 ** 6):
                eng.set_sea(TWO_WAVES)
                want = _from(eng.sea_sample(_tiled(s), n, step, DT), n)
                eng.set_sea(sym.sea(m, TWO_WAVES))
                got = _from(eng.sea_sample(_tiled(s_g), n, step, DT), n)
                bad = sym.differing(got, sym.sea_sample(m, want))
                assert not bad.any(), ("sea_sample", n, m, step, int(bad.sum()))
                assert np.isfinite(want).all() and want[:, 0].any()
            want = _from(eng.mooring_wrench(_tiled(s), _tiled(m9), n), n)
            got = _from(eng.mooring_wrench(_tiled(s_g), _tiled(sym.mooring(m, m9)), n), n)
            bad = sym.differing(got, sym.wrench(m, want))
            assert not bad.any(), ("mooring_wrench", n, m, int(bad.sum()))
            assert want.any(axis=1).mean() >= 0.25
    print(f"[probes {coeff}] hydro_sea_sample (steps 0 and 10^6) and hydro_mooring_wrench, n = 200 and 321, 3 maps: 0 differ")


@COEFFS
def test_seabed_probe_single_corner_exact_the_others_within_twice_the_probe_bound(coeff, bed_pop, engines):
    """The bed population with tilted_boxes of tests/test_symmetry.py (its shares are asserted there, on the CPU).  At most one
    contributing corner on the body and on its image: exact.  The others: |image of the image's wrench - wrench| in units of
    2^-24 of seabed_reference.wrench_scales, against 2 x PROBE_BOUND."""
    st, pv, params, _, _ = bed_pop
    st, _, _ = tilted_boxes(st, pv, params["f32"])
    pr = params[coeff]
    worst, exact, bounded = 0.0, 0, 0
    for n in SIZES:
        eng = engines("designed", pr[:n], coeff)
        eng.set_seabed(BED)
        s = st[:n]
        want = _from(eng.seabed_wrench(_tiled(s), n), n)
        scale = br.wrench_scales(BED, s, pr[:n], br.touching_fp32(BED, s, pr[:n]))
        for m in sym.MAPS:
            s_g = sym.state(m, s)
            got = sym.wrench(m, _from(eng.seabed_wrench(_tiled(s_g), n), n))
            count = np.maximum(contributing_corners(s, pr[:n]), contributing_corners(s_g, pr[:n]))
            single = count <= 1
            bad = sym.differing(got[single], want[single])
            assert not bad.any(), (n, m, int(bad.sum()), np.nonzero(single)[0][bad][:8])
            assert np.isfinite(got).all() and (want[count == 1] != 0).any(axis=1).mean() > 0.5        # (a corner that leaves fast enough bears nothing)
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.where(got == want, 0.0, np.abs(got.astype(np.float64) - want) / (br.ULP * scale))[~single]
            worst = max(worst, float(err.max()))
            exact, bounded = exact + int(single.sum()), bounded + int((~single).sum())
            assert (count == 1).mean() >= 0.25 and (~single).mean() >= 0.10
    print(f"[seabed probe {coeff}] compared exactly {exact}, two or more corners {bounded}: largest difference {worst:.2f} units of 2^-24 of the scale "
          f"(bound 2 x {PROBE_BOUND:g})")
    assert worst <= 2 * PROBE_BOUND


# ---- (d) the resident policies -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resident_pops(pop):
    """name -> (state, prev, params, applied, control, lines): `designed` as the mooring tests draw it; `reseated`: tilted_boxes
    and, for the bodies it moved, the lines drawn anew from the moved state (line_population builds every line from its
    body's own state; the ties at bodies 0 .. 7 are not moved)."""
    st, pv, params, applied, ctl, rec = pop
    moved, _, _ = tilted_boxes(st, pv, params["f32"])
    again = line_population(moved, params["f32"])
    changed = (moved[:, 2] != st[:, 2])
    lines = np.where(changed[:, None], again, rec)
    # the controller's targets follow the body in z, so that the law's terms keep their sizes
    c2 = ctl.copy()
    c2[:, 2] = (ctl[:, 2].astype(np.float64) + (moved[:, 2].astype(np.float64) - st[:, 2])).astype(np.float32)
    return {"designed": (st, pv, params, applied, ctl, rec), "reseated": (moved, pv, params, applied, c2, lines)}


ENTRIES = ("rec", "app-world", "app-body", "ctl", "ctl+app", "sea", "bed", "moor", "ext", "all", "all-far")
WITH_BED = ("bed", "moor", "ext", "all")
LATER = ("teth", "net", "peak", "spread", "irr")                  # the rungs behind _ext: each launched with everything it takes
TOP = ("stat", "ens", "fd", "shear")                              # the rungs behind _irr: everything _irr takes and a statistics record
CHANNEL_PAIRS = ((stx.Z, stx.TENSION), (stx.X, stx.VY))           # nothing flips under any map; each flips under two maps


def _wrong_hand(m, what, net, sea, profile=None):
    """(net, sea, profile): the images of the scene's `net`, `sea` and `profile` under m with ONE of them of the wrong hand, for the
    teeth.  `tether`: every fairlead of the net turned like an axial vector (under the half turn, where polar and axial vectors
    turn alike: left unturned); `ky`: the sea's ky left as the scene has it (a spectrum keeps its depth); `profile`: the
    profile's V_l turned like an axial vector; ("member", k): member k of the ensemble left as the scene has it."""
    net_g, sea_g, profile_g = sym.net(m, net), sym.sea(m, sea), None if profile is None else sym.current_profile(m, profile)
    if what == "tether":
        hand = sym.AXIAL[m] if m != "half_turn" else sym.SAME3
        for l in range(net.shape[1] // 7):
            net_g[:, 7 * l:7 * l + 3] = sym._times(net[:, 7 * l:7 * l + 3], hand)
    elif what == "ky":
        wrong = type(sea)(sea_g.current, sea.depth) if hasattr(sea, "depth") else type(sea)(sea_g.current)
        for (a, kx, _, om, ph), (_, _, ky, _, _) in zip(sea_g.waves, sea.waves):
            wrong.add_wave(a, kx, ky, om, ph)
        sea_g = wrong
    elif what == "profile":
        profile_g = type(profile)(profile.z, sym._times(profile.v, sym.AXIAL[m] if m != "half_turn" else sym.SAME3))
    elif what[0] == "member":
        members = list(sea_g.members)
        members[what[1]] = sea.members[what[1]]
        sea_g = type(sea)(members, sea.bodies_per_sea)
    else:
        raise ValueError(what)
    return net_g, sea_g, profile_g


def _levels_near(st, channels):
    """(n, 2) fp32 levels near the initial values of the two channels (the tension's: near 0): some above, some below, some equal."""
    rng = np.random.default_rng(37)
    lev = np.stack([np.zeros(len(st), np.float32) if c == stx.TENSION else st[:, stx.STATE_FIELD[c]] for c in channels], axis=1)
    return (lev + rng.choice(np.array([-1e-3, 0.0, 1e-3], np.float32), size=lev.shape)).astype(np.float32)


def _resident(eng, entry, P, n, steps, implicit, m=None, bed=BED, wrong=None, sea=None, profile=None, channels=CHANNEL_PAIRS[0]):
    """One launch of `entry` on the population P (m: on its image under that map), every body watched and every step
    recorded with its wrench; returns the outputs MAPPED BACK (the image of the image's outputs): dict of state, prev_out,
    log (steps, n, 19), and where the entry has them extremes, ke and the link tensions (peaks).  The LATER entries take two
    more records of P - the tether net (all bodies, all layers: cut to n by tether_net_population.net_for) and the mooring spread -
    and the bed they run over (`bed`); `wrong`: see _wrong_hand.  The TOP entries take all of that and a statistics record of
    `channels`, reset, against levels near the scene's initial values (the image's: symmetry.levels of them); the record comes
    back as `stat`, symmetry.statistics_words of symmetry.statistics of it, with `left_out`, the columns that are not
    comparable.  `sea`: what the entry steps through - _stat a spectrum (default: the 64 components), _ens an ensemble, _fd and
    _shear a spectrum or an ensemble with a depth; `profile`: _shear's."""
    st, pv, params, applied, ctl, rec = (x if isinstance(x, dict) else x[:n] for x in P[:6])
    top = entry in TOP
    later = entry in LATER or top
    net = net_for(P[6], n, 1 if entry == "teth" else symmetry_population.NET_LAYERS) if later else None
    spread = np.ascontiguousarray(P[7][:n, 0:9 * symmetry_population.SPREAD_LAYERS]) if later else None
    ident = m is None
    if sea is None:
        sea = FULL if entry in ("irr", "stat") else SEA
    lev = _levels_near(st, channels) if top else None
    if not ident:
        st, pv, applied, ctl, rec = sym.state(m, st), sym.prev(m, pv), sym.applied(m, applied), sym.control(m, ctl), sym.mooring(m, rec)
        if wrong is not None:
            net, sea, profile = _wrong_hand(m, wrong, net, sea, profile)
        else:
            net, sea = (sym.net(m, net) if later else None), sym.sea(m, sea)
            profile = None if profile is None else sym.current_profile(m, profile)
        spread = sym.spread(m, spread) if later else None
        lev = sym.levels(m, lev, channels) if top else None
    eng.set_watch(list(range(n)))
    cur, old = _buffers(st, pv, n)
    log = torch.full((steps, 19, n), NAN, dtype=torch.float32, device=DEV)
    a, c17, m9 = _tiled(applied), _tiled(ctl), _tiled(rec)
    kw = dict(implicit_drag=implicit)
    rk = dict(log=log, every=1, phase=1, row0=0)
    ke = record = peaks = stat = None
    _no_water(eng)
    eng.set_seabed(None)
    if entry == "rec":
        eng.step_fused_tiled_multi_rec(cur, old, n, DT, steps, log, 1, 1, 0, **kw)
    elif entry in ("app-world", "app-body"):
        eng.step_fused_tiled_multi_applied(cur, old, n, DT, steps, a, entry[4:], **rk, **kw)
    elif entry in ("ctl", "ctl+app"):
        eng.step_fused_tiled_multi_controlled(cur, old, n, DT, steps, c17, a if entry == "ctl+app" else None, "body", **rk, **kw)
    elif entry == "sea":
        eng.set_sea(sea)
        eng.step_fused_tiled_multi_sea(cur, old, n, DT, steps, STEP0, **rk, **kw)
    elif entry == "bed":
        eng.set_seabed(BED)
        eng.step_fused_tiled_multi_bed(cur, old, n, DT, steps, STEP0, **rk, **kw)
    elif entry == "moor":
        eng.set_sea(sea)
        eng.set_seabed(BED)
        eng.step_fused_tiled_multi_moor(cur, old, n, DT, steps, STEP0, m9, **rk, **kw)
    elif later:
        # everything the entry takes: log, body-frame applied wrench, pose hold, sea (irr: the 64-component spectrum), bed, lines
        # (spread, irr: the spread of three), extremes seeded from the state, the net (teth: one layer), link tensions, ke_out
        # (the TOP entries: and the statistics record; _ens the ensemble, _fd and _shear the finite-depth sea, _shear the profile)
        if entry in ("irr", "stat"):
            eng.set_sea_spectrum(sea)
        elif entry == "ens":
            eng.set_sea_ensemble(sea)
        elif entry in ("fd", "shear"):
            eng.set_sea_finite_depth(sea, n)
            eng.set_current_profile(profile if entry == "shear" else None)
        else:
            eng.set_sea(sea)
        eng.set_seabed(bed)
        record = torch.full((eng.tiles(n), 8, 64), NAN, dtype=torch.float32, device=DEV)
        eng.extremes_reset(record, n, cur)
        ke = _ke()
        t7 = _tiled(net)
        tail = dict(control=c17, applied=a, frame="body", ke_out=ke, **rk, **kw)
        if entry == "teth":
            eng.step_fused_tiled_multi_teth(cur, old, n, DT, steps, STEP0, t7, record, m9, **tail)
        elif entry == "net":
            eng.step_fused_tiled_multi_net(cur, old, n, DT, steps, STEP0, t7, net.shape[1] // 7, record, m9, **tail)
        else:
            peaks = eng.alloc_tiled(net.shape[1] // 7, n)
            if entry == "peak":
                eng.step_fused_tiled_multi_peak(cur, old, n, DT, steps, STEP0, t7, net.shape[1] // 7, peaks, record, m9, **tail)
            elif top:
                stat = eng.statistics_reset(torch.full((eng.tiles(n), nat.STAT_FIELDS, 64), NAN, dtype=torch.float32, device=DEV), n)
                step = getattr(eng, "step_fused_tiled_multi_" + entry)
                step(cur, old, n, DT, steps, STEP0, stat, _tiled(lev), channels[0], channels[1], _tiled(spread), spread.shape[1] // 9, t7,
                     net.shape[1] // 7, peaks, record, **tail)
            else:
                step = eng.step_fused_tiled_multi_irr if entry == "irr" else eng.step_fused_tiled_multi_spread
                step(cur, old, n, DT, steps, STEP0, _tiled(spread), spread.shape[1] // 9, t7, net.shape[1] // 7, peaks, record, **tail)
    else:
        eng.set_sea(sea)
        eng.set_seabed(FAR if entry == "all-far" else BED)
        record = torch.full((eng.tiles(n), 8, 64), NAN, dtype=torch.float32, device=DEV)
        if entry == "ext":
            eng.extremes_reset(record, n)
            eng.step_fused_tiled_multi_ext(cur, old, n, DT, steps, STEP0, record, m9, **rk, **kw)
        else:
            eng.extremes_reset(record, n, cur)
            ke = _ke()
            eng.step_fused_tiled_multi_ext(cur, old, n, DT, steps, STEP0, record, m9, c17, a, "body", ke_out=ke, **rk, **kw)
    torch.cuda.synchronize()
    out = {"state": _from(old, n), "prev_out": _from(cur, n)[:, 7:13], "log": np.ascontiguousarray(_np(log).transpose(0, 2, 1))}
    if record is not None:
        out["extremes"] = _from(record, n)
    if ke is not None:
        out["ke"] = _np(ke)
    if peaks is not None:
        out["peaks"] = _from(peaks, n)                               # scalars: the image's are the scene's
    if stat is not None:
        words = stx.unpack(_np(stat), n)
        out["stat"] = sym.statistics_words(words if ident else sym.statistics(m, words, channels))
        out["left_out"] = [] if ident else sym.statistics_left_out(m, channels)
    if later:
        _no_water(eng)
    if not ident:
        out["state"], out["prev_out"], out["log"] = sym.state(m, out["state"]), sym.prev(m, out["prev_out"]), sym.log_row(m, out["log"])
        if record is not None:
            out["extremes"] = sym.extremes(m, out["extremes"])
    return out, st


def _sensitive_from(st0, log, pr, bed=BED):
    """(n,) the first step (0-based row) whose INPUT state has two or more contributing corners on `bed`; `steps` if none has.
    The input of row 0 is st0, of row j the state row j - 1 recorded."""
    steps, n = log.shape[0], log.shape[1]
    first = np.full(n, steps)
    for j in range(steps - 1, -1, -1):
        s = st0 if j == 0 else log[j - 1, :, 0:13]
        with np.errstate(all="ignore"):
            many = contributing_corners(np.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0), pr, bed) >= 2
        first = np.where(many, j, first)
    return first


def _compare(entry, want, got, first, what):
    """Exact where the reference calls the body order-insensitive; returns (bodies compared exactly through the last step,
    bodies left out)."""
    steps, n = want["log"].shape[0], want["log"].shape[1]
    for j in range(steps):
        live = first > j
        bad = sym.differing(got["log"][j][live], want["log"][j][live])
        assert not bad.any(), what + ("log row", j, int(bad.sum()), np.nonzero(live)[0][bad][:8])
    whole = first >= steps
    for k in ("state", "prev_out", "extremes", "peaks", "stat"):
        if k in want:
            a, b = got[k], want[k]
            if k == "stat":                                         # the up-crossing word of a flipped slot: left out on both sides
                a, b = a.copy(), b.copy()
                a[:, got["left_out"]], b[:, got["left_out"]] = 0.0, 0.0
            bad = sym.differing(a[whole], b[whole])
            assert not bad.any(), what + (k, int(bad.sum()), np.nonzero(whole)[0][bad][:8])
    if "ke" in want and whole.all():
        assert sym.equal(got["ke"], want["ke"]), what + ("ke", got["ke"], want["ke"])
    assert sym.equal(want["log"][steps - 1][:, 0:13], want["state"]), what                                                # the last row is the final state
    return int(whole.sum()), int((~whole).sum())


def _one_step_scales(entry, st, pv, pr, coeff, implicit, wrench):
    """field_scales of the step the device made: its own logged wrench, and with implicit drag the drag coefficients of the
    oracle on the state the wrench saw (relative to the sea, where there is one)."""
    k = None
    if implicit:
        s_rel, pv_rel = st, pv
        if entry in ("moor", "ext", "all"):
            eta, u = sr.water(SEA, st[:, 0], st[:, 1], st[:, 2], STEP0, DT)
            s_rel, pv_rel = sr.relative(st, pv, eta.astype(np.float32), u.astype(np.float32))
        comps = ho.step_wrench(s_rel, pv_rel, io._coeffs(pr, coeff), RHO, G, DT)[2]
        k = io.drag_jacobian(s_rel, pr, comps, RHO, coeff)
    return k, wrench.astype(np.float64)


@COEFFS
@DRAG
@pytest.mark.parametrize("which", ["designed", "reseated"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_resident_policies_are_exactly_symmetric(entry, which, coeff, implicit, resident_pops, engines):
    """_rec, _app (world and body frame), _ctl (without and with a body-frame applied wrench), _sea (waves + current), _bed,
    _moor and _ext (over sea and bed), and the everything-on _ext launch (log, body-frame applied wrench, pose hold, sea, bed,
    lines, extremes seeded from the state, ke_out; `all-far`: the same over a bed nobody reaches, where the energy pair can
    be compared), each at 1 and 7 steps, n = 200 and 321, under the three maps."""
    P = resident_pops[which]
    pr = P[2][coeff]
    Pc = (P[0], P[1], pr, P[3], P[4], P[5])
    report = []
    for n in SIZES:
        eng = engines("designed", pr[:n], coeff)
        for steps in STEPS:
            want, st0 = _resident(eng, entry, Pc, n, steps, implicit)
            assert not sym.equal(want["state"], st0)
            bed = entry in WITH_BED
            first0 = _sensitive_from(st0, want["log"], pr[:n]) if bed else np.full(n, steps)
            fewest, most, one_step = n, 0, None
            for m in sym.MAPS:
                got, st_g = _resident(eng, entry, Pc, n, steps, implicit, m)
                first = np.minimum(first0, _sensitive_from(sym.state(m, st_g), got["log"], pr[:n])) if bed else first0
                exact, left = _compare(entry, want, got, first, (entry, which, n, steps, m))
                fewest, most = min(fewest, exact), max(most, left)
                out = first < steps
                if bed and implicit:
                    for j in range(steps):                          # left out, but finite
                        gone = first <= j
                        assert np.isfinite(got["log"][j][gone]).all() and np.isfinite(want["log"][j][gone]).all(), (entry, which, n, steps, m, j)
                if bed and steps == 1 and out.any():
                    k, w = _one_step_scales(entry, st0, Pc[1][:n], pr[:n], coeff, implicit, want["log"][0][:, 13:19])
                    kk = None if k is None else (k[0][out], k[1][out])
                    ref = want["state"][out].astype(np.float64)
                    sc = io.field_scales(st0[out], w[out], pr[:n][out], G, DT, kk, ref)
                    err = io.integrator_error_ulps(got["state"][out], ref, st0[out], w[out], pr[:n][out], G, DT, kk, scales=sc)
                    worst = io.max_error_ulps(err)
                    one_step = max(one_step or 0.0, worst)
                    assert worst <= 2 * io.STEP_ULP_BOUND, (entry, which, n, m, worst)
                if which == "reseated" and steps == 7 and implicit:
                    assert left <= 0.25 * n, (entry, n, m, left)
            report.append(f"n={n} x{steps}: {fewest} exact, {most} left out ({most / n:.0%})"
                          + (f", their one step within {one_step:.2f} ulps of its image (bound 2 x {io.STEP_ULP_BOUND:g})" if one_step is not None else ""))
    print(f"[resident {entry} {which} {coeff} {'implicit' if implicit else 'explicit'}, fewest / most over the 3 maps] " + "; ".join(report))


@COEFFS
@DRAG
@pytest.mark.parametrize("variant", ["non_temporal", "warp"])
def test_everything_on_non_temporal_and_warp(variant, coeff, implicit, resident_pops, engines):
    """The everything-on launch with non_temporal = 1, and under Warp semantics (the engine's settings; `_resident` leaves
    them alone)."""
    P = resident_pops["reseated"]
    pr = P[2][coeff]
    Pc = (P[0], P[1], pr, P[3], P[4], P[5])
    shown = []
    for n in SIZES:
        eng = engines("designed", pr[:n], coeff)
        if variant == "warp":
            eng.set_semantics("warp")
        else:
            eng.set_tuning(0, 0, 1)
        for entry in ("all", "all-far"):
            for steps in STEPS:
                want, st0 = _resident(eng, entry, Pc, n, steps, implicit)
                bed = entry == "all"
                first0 = _sensitive_from(st0, want["log"], pr[:n]) if bed else np.full(n, steps)
                for m in sym.MAPS:
                    got, st_g = _resident(eng, entry, Pc, n, steps, implicit, m)
                    first = np.minimum(first0, _sensitive_from(sym.state(m, st_g), got["log"], pr[:n])) if bed else first0
                    exact, left = _compare(entry, want, got, first, (variant, entry, n, steps, m))
                    if steps == 7 and n == 321:
                        shown.append(f"{entry} {m}: {exact} exact, {left} left out")
    print(f"[everything on, {variant} {coeff} {'implicit' if implicit else 'explicit'}] n=321 steps=7 " + "; ".join(shown))


# ---- (e) the later rungs: tether, net, link tensions, spread, irregular sea ------------------------------------------------------------
@pytest.fixture(scope="module")
def later_pop(bed_pop):
    """tests/symmetry_population.py (its shares are asserted in tests/test_symmetry.py, on the CPU) with the bed population's
    applied wrench and control record, the targets following the bodies in z: (state, prev, params, applied, control, lines,
    net (322, 28), spread (321, 36))."""
    _, _, params, applied, ctl = bed_pop
    P = symmetry_population.reseated_population()
    assert all(np.array_equal(P["params"][c], params[c]) for c in ("f32", "f16"))
    return (P["st"], P["pv"], P["params"], applied, symmetry_population.follow(ctl, P["drawn"], P["st"]), P["lines"], P["net"], P["spread"])


@COEFFS
def test_tether_spread_and_spectrum_probes_are_exactly_symmetric(coeff, later_pop, engines):
    """hydro_tether_wrench (wrench and tension) on each of the net's two layers, hydro_mooring_wrench on every layer of the spread
    (mooring_spread_wrench) and hydro_sea_spectrum_sample at 11 and 64 components and steps 0 and 10^6: the image's output is the
    image of the output, tensions and eta keep their bits.  Alongside, what makes that say something: at least 20 % of the bodies
    are pulled in each layer of the net, at least 30 % in each of the spread's layers 0 and 1, and eta is non-zero."""
    st, _, params, _, _, _, net_all, spread_all = later_pop
    for n in SIZES:
        eng = engines("designed", params[coeff][:n], coeff)
        s, net, spread = st[:n], net_for(net_all, n, symmetry_population.NET_LAYERS), spread_all[:n]
        W, T = eng.tether_net_wrench(_tiled(s), _tiled(net), n, 2)
        W, T = [_from(w, n) for w in W], [_from(t, n)[:, 0] for t in T]
        S = [_from(w, n) for w in eng.mooring_spread_wrench(_tiled(s), _tiled(spread), n, 4)]
        assert all((t > 0).mean() >= 0.2 for t in T), n
        assert all(w.any(axis=1).mean() >= 0.3 for w in S[:2]) and S[2].any() and not S[3].any(), n
        for m in sym.MAPS:
            s_g = sym.state(m, s)
            W_g, T_g = eng.tether_net_wrench(_tiled(s_g), _tiled(sym.net(m, net)), n, 2)
            for l in range(2):
                bad = sym.differing(_from(W_g[l], n), sym.wrench(m, W[l])) | sym.differing(_from(T_g[l], n)[:, 0], T[l])
                assert not bad.any(), ("tether_wrench", n, m, l, int(bad.sum()), np.nonzero(bad)[0][:8])
            for l, w_g in enumerate(eng.mooring_spread_wrench(_tiled(s_g), _tiled(sym.spread(m, spread)), n, 4)):
                bad = sym.differing(_from(w_g, n), sym.wrench(m, S[l]))
                assert not bad.any(), ("mooring_spread_wrench", n, m, l, int(bad.sum()), np.nonzero(bad)[0][:8])
            for count in (11, 64):
                spec = ssr.truncated(FULL, count)
                for step in (0, 10 ** 6):
                    eng.set_sea_spectrum(spec)
                    want = _from(eng.sea_spectrum_sample(_tiled(s), n, step, DT), n)
                    eng.set_sea_spectrum(sym.sea(m, spec))
                    got = _from(eng.sea_spectrum_sample(_tiled(s_g), n, step, DT), n)
                    bad = sym.differing(got, sym.sea_sample(m, want))
                    assert not bad.any(), ("sea_spectrum_sample", n, m, count, step, int(bad.sum()), np.nonzero(bad)[0][:8])
                    assert np.isfinite(want).all() and want[:, 0].all()
            eng.set_sea_spectrum(None)
    print(f"[probes {coeff}] hydro_tether_wrench (2 layers, wrench and tension), mooring_spread_wrench (4 layers) and hydro_sea_spectrum_sample "
          "(11 and 64 components, steps 0 and 10^6), n = 200 and 321, 3 maps: 0 differ")


def _later(eng, entry, P, pr, n, steps, implicit, bed, what, **water):
    """The launch of `entry` on P and on its three images, compared by `_compare`: [(map, bodies exact, bodies left out)].  A body
    is left out from the first step whose input state has two or more contributing corners ON THE BED THAT IS SET, on the scene
    or on the image (_sensitive_from: the reference decides).  Over FAR that is nobody - but for a body that explicit drag has
    carried out of the scene: FAR is a plane at z = -10^6 m, and seven explicit steps take light bodies to 10^14 m and beyond
    (the module's docstring), eight corners below any plane.  The callers assert that this happens under explicit drag only.
    `water`: the sea, profile and channels of a TOP entry (see _resident)."""
    want, st0 = _resident(eng, entry, P, n, steps, implicit, bed=bed, **water)
    assert not sym.equal(want["state"], st0)
    first0 = _sensitive_from(st0, want["log"], pr[:n], bed)
    out = []
    for m in sym.MAPS:
        got, st_g = _resident(eng, entry, P, n, steps, implicit, m, bed=bed, **water)
        first = np.minimum(first0, _sensitive_from(sym.state(m, st_g), got["log"], pr[:n], bed))
        exact, left = _compare(entry, want, got, first, what + (n, steps, m))
        if implicit:                                                # left out, but finite
            gone = first < steps
            assert np.isfinite(got["log"][:, gone]).all() and np.isfinite(want["log"][:, gone]).all(), what + (n, steps, m)
        out.append((m, exact, left))
    if implicit:
        # the launch did what its name says: the lines pulled (tension_max), and where there are link tensions every layer of the net did
        assert (want["extremes"][:, 7] > 0).mean() >= 0.3 and np.isfinite(want["ke"]).all(), what + (n, steps)
        assert "peaks" not in want or ((want["peaks"] > 0).mean(axis=0) >= 0.2).all(), what + (n, steps)
        # and the record holds what the launch sampled: n = steps for every body, both S2 non-zero for at least half of them
        assert "stat" not in want or ((want["stat"][:, 6] == steps).all() and (want["stat"][:, [1, 3]] > 0).all(axis=1).mean() >= 0.5), what + (n, steps)
    return out


@COEFFS
@DRAG
@pytest.mark.parametrize("over", ["far", "bed"])
@pytest.mark.parametrize("entry", LATER)
def test_later_rungs_are_exactly_symmetric(entry, over, coeff, implicit, later_pop, engines):
    """_teth, _net, _peak, _spread and _irr, each with everything it takes switched on: the log of every body with its wrench, a
    body-frame applied wrench and the pose hold, the sea (SEA; _irr: the 64-component spectrum), the bed, the lines (_spread and
    _irr: the spread of three), extremes seeded from the state, the net (_teth: one layer; the others two), the link tensions
    (from _peak on) and ke_out; n = 200 and 321, under the three maps.
      over FAR, a bed nobody reaches, at 1 and 7 steps: EVERY body exact in every log row, in state, prev_out and the extremes
        record; the link tensions and the energy pair the same bits (with explicit drag a NaN equals a NaN).  Nobody is left out:
        asserted at 1 step, and at 7 steps under implicit drag.  Seven EXPLICIT steps throw light bodies out of the scene (the
        module's docstring), through FAR's plane at z = -10^6 m as through any other: such a body, eight corners below FAR by
        the reference, is left out from that step on by the rule of the bed's corner sum - the one found (body 78 at n = 200, in
        the sixth step at z = -5.4e14 m, its recorded wrench FAR's spring and damper at 1.9e17 N) differs from its image by one
        ulp in that wrench and in nothing else.
      over BED, ONE step: the bodies with at most one contributing corner on the scene and on the image exact; the others left out,
        finite under implicit drag, and at most 25 % of the bodies.
    Several steps over BED are deliberately not run for these rungs: a tether hands an order-sensitive body's last-bit difference to
    its partner on the next step, that one to its own partner in the other layer on the step after, so the set that may be left
    out grows along the chains and rings of the net by a link per step - the test would hide what it is meant to show.  In ONE step
    every line is formed from the input states, which are exact images, so a tethered partner of an order-sensitive body is still
    compared exactly."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    pr = P[2]
    bed = BED if over == "bed" else FAR
    report = []
    for n in SIZES:
        eng = engines("designed", pr[:n], coeff)
        for steps in (STEPS if over == "far" else (1,)):
            runs = _later(eng, entry, P, pr, n, steps, implicit, bed, (entry, over))
            fewest, most = min(r[1] for r in runs), max(r[2] for r in runs)
            if over == "bed":
                assert most <= 0.25 * n, (entry, over, n, steps, most)
            else:                                                   # nobody reaches FAR - unless explicit drag has thrown it out of the scene
                assert most == 0 or (not implicit and steps > 1 and most <= 0.25 * n), (entry, over, n, steps, most)
            report.append(f"n={n} x{steps}: {fewest} exact, {most} left out ({most / n:.0%}), 0 differ")
    print(f"[resident {entry} over {over.upper()} {coeff} {'implicit' if implicit else 'explicit'}, fewest / most over the 3 maps] " + "; ".join(report))


@COEFFS
@DRAG
@pytest.mark.parametrize("variant", ["non_temporal", "warp"])
def test_irregular_sea_everything_on_non_temporal_and_warp(variant, coeff, implicit, later_pop, engines):
    """The everything-on _irr launch over FAR, 7 steps, n = 321, with non_temporal = 1 and under Warp semantics (the engine's
    settings; `_resident` leaves them alone)."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    n = 321
    eng = engines("designed", P[2][:n], coeff)
    if variant == "warp":
        eng.set_semantics("warp")
    else:
        eng.set_tuning(0, 0, 1)
    runs = _later(eng, "irr", P, P[2], n, 7, implicit, FAR, (variant, "irr"))
    assert not implicit or all(left == 0 for _, _, left in runs)    # (explicit: a body thrown below FAR's plane, see _later)
    print(f"[irr, everything on, {variant} {coeff} {'implicit' if implicit else 'explicit'}] n=321 steps=7 "
          + "; ".join(f"{m}: {exact} exact, {left} left out, 0 differ" for m, exact, left in runs))


@COEFFS
def test_teeth_on_the_device_wrong_hand_images_are_told_apart(coeff, later_pop, engines):
    """Two images of the wrong hand through the same launches and the same comparison (state, prev_out or any log row): the
    net's fairleads turned like axial vectors (_net, every map; under the half turn left unturned) and the spectrum's ky not
    flipped under mirror_y (_irr).  At least a quarter of the bodies must differ from the predicted image - and with the right
    hand none does.  One implicit step over FAR."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    shown = []
    for n in SIZES:
        eng = engines("designed", P[2][:n], coeff)
        for entry, wrong, maps in (("net", "tether", sym.MAPS), ("irr", "ky", ("mirror_y",))):
            want, _ = _resident(eng, entry, P, n, 1, True, bed=FAR)
            for m in maps:
                def apart(got):
                    return sym.differing(got["state"], want["state"]) | sym.differing(got["prev_out"], want["prev_out"]) | sym.differing(got["log"][0], want["log"][0])
                assert not apart(_resident(eng, entry, P, n, 1, True, m, bed=FAR)[0]).any(), (entry, n, m)
                share = apart(_resident(eng, entry, P, n, 1, True, m, bed=FAR, wrong=wrong)[0]).mean()
                shown.append(f"{wrong} {m} n={n}: {share:.0%}")
                assert share >= 0.25, (entry, wrong, n, m, share)
    print(f"[teeth on the device {coeff}] bodies that differ from the predicted image: " + "; ".join(shown))


# ---- (g) statistics, ensembles, finite depth and the sheared current --------------------------------------------------------------------
H = symmetry_population.FD_DEPTH                                  # the depth the resident rungs run at (tests/symmetry_population.py)


def _top_water(case, n):
    """(entry, dict(sea, profile)) of a case of the TOP rungs at n bodies."""
    one = symmetry_population.fd_sea()
    return {
        "stat": ("stat", dict(sea=FULL)),
        "ens-1": ("ens", dict(sea=seh.ensemble(64, n, 1))),                  # every wavefront reads its own member
        "ens-4": ("ens", dict(sea=seh.ensemble(64, n, 4))),                  # a block shares one member; the last member lies partly past n
        "fd-one": ("fd", dict(sea=one)),                                     # the designed sea as an ensemble of one
        "fd-ens": ("fd", dict(sea=symmetry_population.fd_ensemble(64, n, 1))),
        "shear-16": ("shear", dict(sea=one, profile=cpr.turning_profile(16, depth=H))),
        "shear-2": ("shear", dict(sea=symmetry_population.fd_ensemble(64, n, 4), profile=cpr.turning_profile(2, depth=H))),
    }[case]


TOP_CASES = ("stat", "ens-1", "ens-4", "fd-one", "fd-ens", "shear-16", "shear-2")


@COEFFS
def test_ensemble_depth_and_profile_probes_are_exactly_symmetric(coeff, later_pop, engines):
    """hydro_sea_ensemble_sample (tiles_per_sea 1 and 4), hydro_sea_finite_depth_sample (a spectrum as an ensemble of one, and an
    ensemble) and hydro_current_profile_sample (without a profile, with 2 and with 16 knots), at 11 and 64 components and steps 0
    and 10^6: the image's sample is symmetry.sea_sample of the sample and eta keeps its bits.  Populations: tests/
    symmetry_population.py at n = 200 and 321 in FD_DEPTH of water; sea_depth_reference.population() (130 bodies over the whole
    column of 9 m: both clamps and the inside, asserted in tests/test_symmetry.py); and for the profile
    symmetry_population.knot_population, a body in every knot interval."""
    st, _, params = later_pop[0], later_pop[1], later_pop[2]
    column = sdr.population()
    pops = [("reseated", st[:n], H, "designed") for n in SIZES] + [("column", column, sdr.DEPTH, "column")]
    launches = 0
    for name, s, depth, key in pops:
        n = len(s)
        eng = engines(key, params[coeff][:max(n, 130)], coeff)
        for count in (11, 64):
            one = sdr.designed_sea(count, depth)
            fd_ens = symmetry_population.fd_ensemble(count, n, 1, depth)
            cases = [("ensemble", seh.ensemble(count, n, tps), None, s) for tps in (1, 4)]
            cases += [("finite_depth", one, None, s), ("finite_depth", fd_ens, None, s), ("profile", fd_ens, None, s)]
            for knots in (2, 16):
                profile = cpr.turning_profile(knots, depth=depth)
                cases += [("profile", one, profile, s), ("profile", one, profile, symmetry_population.knot_population(profile, one, 0, DT))]
            for kind, sea, profile, bodies in cases:
                nb = len(bodies)

                def sample(sea_, profile_, bodies_, step):
                    _no_water(eng)
                    if kind == "ensemble":
                        eng.set_sea_ensemble(sea_)
                        return _from(eng.sea_ensemble_sample(_tiled(bodies_), nb, step, DT), nb)
                    eng.set_sea_finite_depth(sea_, nb)
                    if kind == "finite_depth":
                        return _from(eng.sea_finite_depth_sample(_tiled(bodies_), nb, step, DT), nb)
                    eng.set_current_profile(profile_)
                    return _from(eng.current_profile_sample(_tiled(bodies_), nb, step, DT), nb)
                for step in (0, 10 ** 6):
                    want = sample(sea, profile, bodies, step)
                    assert np.isfinite(want).all() and want[:, 0].all() and want[:, 1:4].any(axis=0).all()
                    for m in sym.MAPS:
                        got = sample(sym.sea(m, sea), None if profile is None else sym.current_profile(m, profile), sym.state(m, bodies), step)
                        bad = sym.differing(got, sym.sea_sample(m, want)) | (got[:, 0].view(np.uint32) != want[:, 0].view(np.uint32))
                        assert not bad.any(), (kind, name, nb, count, step, m, None if profile is None else profile.knots, int(bad.sum()), np.nonzero(bad)[0][:8])
                        launches += 1
        _no_water(eng)
    print(f"[probes {coeff}] hydro_sea_ensemble_sample, hydro_sea_finite_depth_sample and hydro_current_profile_sample (none, 2 and 16 knots), 11 and 64 "
          f"components, steps 0 and 10^6, n = 200, 321 and 130 (the profile: and a body in every knot interval), 3 maps: {launches} images, 0 differ")


@COEFFS
@DRAG
@pytest.mark.parametrize("over", ["far", "bed"])
@pytest.mark.parametrize("case", TOP_CASES)
def test_top_rungs_are_exactly_symmetric(case, over, coeff, implicit, later_pop, engines):
    """_stat, _ens, _fd and _shear, each with everything it takes switched on: everything _irr takes in
    test_later_rungs_are_exactly_symmetric and a statistics record, reset, against levels near the initial values, once over the
    channels (z, tension) - nothing flips under any map - and once over (x, vy), which flip under two maps each: S1 -> -S1, S2 and
    n the same bits, the up-crossing word of the flipped slot left out (tests/symmetry.py).  The water: `_top_water`.  The
    expectations are those of test_later_rungs_are_exactly_symmetric, with the statistics record among what is compared:
      over FAR, at 1 and 7 steps: every body exact in every log row, state, prev_out, extremes, link tensions and the record, the
        energy pair the same bits; nobody left out at 1 step nor at 7 implicit steps, at most 25 % after 7 explicit steps;
      over BED, ONE step: the bodies with at most one contributing corner exact, the others left out and at most 25 %."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    pr = P[2]
    bed = BED if over == "bed" else FAR
    report = []
    for n in SIZES:
        eng = engines("designed", pr[:n], coeff)
        entry, water = _top_water(case, n)
        for steps in (STEPS if over == "far" else (1,)):
            for channels in CHANNEL_PAIRS:
                runs = _later(eng, entry, P, pr, n, steps, implicit, bed, (case, over, channels), channels=channels, **water)
                fewest, most = min(r[1] for r in runs), max(r[2] for r in runs)
                if over == "bed":
                    assert most <= 0.25 * n, (case, over, n, steps, most)
                else:
                    assert most == 0 or (not implicit and steps > 1 and most <= 0.25 * n), (case, over, n, steps, most)
            report.append(f"n={n} x{steps}: {fewest} exact, {most} left out ({most / n:.0%}), 0 differ")
    print(f"[resident {case} over {over.upper()} {coeff} {'implicit' if implicit else 'explicit'}, fewest / most over the 3 maps] " + "; ".join(report))


@COEFFS
@DRAG
@pytest.mark.parametrize("variant", ["non_temporal", "warp"])
def test_sheared_current_everything_on_non_temporal_and_warp(variant, coeff, implicit, later_pop, engines):
    """The everything-on _shear launch (16 knots) over FAR, 7 steps, n = 321, with non_temporal = 1 and under Warp semantics,
    both channel pairs."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    n = 321
    eng = engines("designed", P[2][:n], coeff)
    if variant == "warp":
        eng.set_semantics("warp")
    else:
        eng.set_tuning(0, 0, 1)
    entry, water = _top_water("shear-16", n)
    for channels in CHANNEL_PAIRS:
        runs = _later(eng, entry, P, P[2], n, 7, implicit, FAR, (variant, "shear", channels), channels=channels, **water)
        assert all(left == 0 if implicit else left <= 0.25 * n for _, _, left in runs)
    print(f"[shear, everything on, {variant} {coeff} {'implicit' if implicit else 'explicit'}] n=321 steps=7 "
          + "; ".join(f"{m}: {exact} exact, {left} left out, 0 differ" for m, exact, left in runs))


def _reference_water(sea, st, time):
    """(eta, u) in fp64 at `time` seconds of whatever kind of sea: sea_depth_reference.water serves a sea with and without a
    depth; an ensemble goes block by block."""
    if hasattr(sea, "members"):
        eta, u = np.empty(len(st)), np.empty((len(st), 3))
        for k, member in enumerate(sea.members):
            at = slice(k * sea.bodies_per_sea, min((k + 1) * sea.bodies_per_sea, len(st)))
            eta[at], u[at] = _reference_water(member, st[at], time)
        return eta, u
    with np.errstate(all="ignore"):
        return sdr.water(sea, st[:, 0], st[:, 1], st[:, 2], 1, time)


@COEFFS
def test_open_loop_sea_entries_are_exactly_symmetric(coeff, later_pop, wrench_pops, engines):
    """hydro_step_wrench_tiled_sea and hydro_step_wrench_aos_sea (both quaternion orders) under SEA with hydro_sea_sample at a
    time; hydro_step_wrench_tiled_irr, hydro_step_wrench_aos_irr and the matching sample while the engine holds, in turn, the
    64-component spectrum, an ensemble and a finite-depth ensemble - at times 0, 7 dt and 10^6 dt, on edge_cases (81 bodies) and
    tests/symmetry_population.py at n = 321.  The image's wrench is symmetry.wrench of the wrench, the engine-owned previous
    velocity afterwards the image of the scene's, the sample symmetry.sea_sample of the sample.  At least half of the bodies are
    wet by the fp64 water and the oracle."""
    fx = wrench_pops["edge_cases"]
    pops = [("edge_cases",) + fx, ("reseated", later_pop[0], later_pop[1], later_pop[2][coeff], RHO, G, DT)]
    for name, st, pv, pr, rho, g, dt in pops:
        n = len(st)
        eng = engines(name, pr, coeff, rho, g) if name == "edge_cases" else engines("designed", pr[:n], coeff)
        holders = (("sea", SEA), ("spectrum", FULL), ("ensemble", seh.ensemble(64, n, 1)), ("finite depth", symmetry_population.fd_ensemble(64, n, 1)))

        def entries(kind, sea, s, p, time):
            """name -> (n, 6) wrench or (n, 4) sample, and name + ' prev' -> the engine-owned previous velocity after the call."""
            _no_water(eng)
            {"sea": eng.set_sea, "spectrum": eng.set_sea_spectrum, "ensemble": eng.set_sea_ensemble, "finite depth": eng.set_sea_finite_depth}[kind](sea)
            tiled, aos, sample = ((eng.step_wrench_tiled_sea, eng.step_wrench_aos_sea, eng.sea_sample_at) if kind == "sea" else
                                  (eng.step_wrench_tiled_irr, eng.step_wrench_aos_irr, eng.irregular_sea_sample_at))
            out = {"sample": _from(sample(_tiled(s), n, time), n)}
            eng.set_prev_velocity(_soa(p))
            out["tiled"] = _from(tiled(_tiled(s), n, dt, time), n)
            out["tiled prev"] = _np(eng.get_prev_velocity()).T
            pos, vel = _rows(s[:, 0:3]), _rows(s[:, 7:13])
            for which, quat, xyzw in (("aos_wxyz", s[:, [6, 3, 4, 5]], False), ("aos_xyzw", s[:, 3:7], True)):
                eng.set_prev_velocity(_soa(p))
                f, t = aos(pos, _rows(quat), vel, dt, time, quat_xyzw=xyzw)
                out[which] = np.concatenate([_np(f), _np(t)], axis=1)
                out[which + " prev"] = _np(eng.get_prev_velocity()).T
            torch.cuda.synchronize()
            return out
        shown = []
        for kind, sea in holders:
            for time in (0.0, 7 * dt, 10 ** 6 * dt):
                want = entries(kind, sea, st, pv, time)
                eta, u = _reference_water(sea, st, time)
                with np.errstate(all="ignore"):
                    s_rel, pv_rel = sr.relative(st, pv, eta.astype(np.float32), u.astype(np.float32))
                    wet = ho.step_wrench(s_rel, pv_rel, io._coeffs(pr, coeff), rho, g, dt)[2]["ratio"] > 0
                assert wet.mean() >= 0.5, (name, kind, time, wet.mean())
                assert (want["tiled"][wet] != 0).any(axis=1).mean() >= 0.9 and sym.equal(want["tiled prev"], st[:, 7:13])
                for m in sym.MAPS:
                    got = entries(kind, sym.sea(m, sea), sym.state(m, st), sym.prev(m, pv), time)
                    for k, v in want.items():
                        image = sym.sea_sample(m, v) if k == "sample" else sym.prev(m, v) if k.endswith("prev") else sym.wrench(m, v)
                        bad = sym.differing(got[k], image)
                        assert not bad.any(), (name, kind, time, m, k, int(bad.sum()), np.nonzero(bad)[0][:8])
                    known = ~np.isnan(want["sample"][:, 0])                     # eta keeps its BITS (a NaN its being one)
                    assert np.array_equal(got["sample"][known, 0].view(np.uint32), want["sample"][known, 0].view(np.uint32)), (name, kind, time, m)
            shown.append(f"{kind} ({int(wet.sum())} wet)")
        _no_water(eng)
        print(f"[open-loop sea entries {coeff}] {name}: {n} bodies x 3 times x 3 maps x (tiled, aos wxyz, aos xyzw, sample; the previous velocity): "
              + ", ".join(shown) + ": 0 differ")


@COEFFS
def test_teeth_on_the_device_depth_profile_and_member(coeff, later_pop, engines):
    """Three images of the wrong hand through the same launches and the same comparison, one implicit step over FAR: (a) the
    finite-depth sea's ky not flipped under mirror_y (_fd) and (b) the profile's V_l turned like an axial vector under mirror_y
    and mirror_x (_shear): at least a quarter of the bodies differ from the predicted image; (c) ONE member of the ensemble at
    tiles_per_sea = 1 left unturned under mirror_y (_ens): at least a quarter of THAT member's bodies differ and not one body of
    any other member - the comparison resolves the member mapping.  With the right hand none differs in any of the three."""
    P = (later_pop[0], later_pop[1], later_pop[2][coeff]) + later_pop[3:]
    member = 2                                                      # bodies 128 .. 191, at either size
    shown = []
    for n in SIZES:
        eng = engines("designed", P[2][:n], coeff)
        for case, wrong, maps in (("fd-one", "ky", ("mirror_y",)), ("shear-16", "profile", ("mirror_y", "mirror_x")), ("ens-1", ("member", member), ("mirror_y",))):
            entry, water = _top_water(case, n)
            want, _ = _resident(eng, entry, P, n, 1, True, bed=FAR, **water)
            for m in maps:
                def apart(got):
                    return sym.differing(got["state"], want["state"]) | sym.differing(got["prev_out"], want["prev_out"]) | sym.differing(got["log"][0], want["log"][0])
                assert not apart(_resident(eng, entry, P, n, 1, True, m, bed=FAR, **water)[0]).any(), (case, n, m)
                bad = apart(_resident(eng, entry, P, n, 1, True, m, bed=FAR, wrong=wrong, **water)[0])
                if case == "ens-1":
                    mine = water["sea"].sea_of(np.arange(n)) == member
                    assert mine.sum() == 64 and not bad[~mine].any(), (case, n, m, np.nonzero(bad & ~mine)[0][:8])
                    bad = bad[mine]
                shown.append(f"{wrong if isinstance(wrong, str) else 'member'} {m} n={n}: {bad.mean():.0%}")
                assert bad.mean() >= 0.25, (case, wrong, n, m, bad.mean())
    print(f"[teeth on the device, depth, profile and member {coeff}] bodies that differ from the predicted image: " + "; ".join(shown))


# ---- (f) ClosedLoopSim ------------------------------------------------------------------------------------------------------------------
def test_closed_loop_sim_builds_its_records_without_a_hand(native_built):
    """64 moored buoys at 64 headings, a current with one wave component, an off-centre fairlead and a weak pose hold towards a
    displaced, turned target - and the mirror_y image of all of it, both through ClosedLoopSim's own set_mooring / set_pose_hold
    / set_sea: run_resident(20, chunk=7) with track_extremes leaves the image's final state and Extremes the images of the
    scene's."""
    sc, anchors, z_eq, mass = _buoys()
    k, c = Mooring.for_body(mass, sc.dt)
    sea = SeaState((0.5, -0.2, 0.0)).add_wave(0.3, 0.21, 0.13, 1.55, 0.7)
    rng = np.random.default_rng(9)
    fairlead = np.array([0.05, 0.02, -0.05])
    target_p = sc.state[:, 0:3].astype(np.float64) + rng.uniform(-0.5, 0.5, (sc.n, 3))
    axis = rng.normal(size=(sc.n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.1, 0.6, (sc.n, 1))
    target_q = np.concatenate([np.sin(half) * axis, np.cos(half)], axis=1).astype(np.float32)
    L0 = DEPTH - 0.2                                                # taut from the first step
    m = "mirror_y"
    polar = np.asarray(sym.POLAR[m], np.float64)
    finals, records = {}, {}
    for name in ("scene", "image"):
        im = name == "image"
        scene = scenes.Scene("buoys", sym.state(m, sc.state), sym.prev(m, sc.prev), sc.params, dt=sc.dt, rho=sc.rho, g=sc.g) if im else sc
        sim = ClosedLoopSim(scene, implicit_drag=True)
        sim.set_sea(sym.sea(m, sea) if im else sea)
        sim.set_mooring(anchors * polar if im else anchors, fairlead * polar if im else fairlead, length=L0, stiffness=k, damping=c)
        sim.set_pose_hold(position=(target_p * polar if im else target_p).astype(np.float32),
                          orientation_xyzw=sym._times(target_q, sym.QUAT[m]) if im else target_q,
                          kp_lin=2.0 * mass, kd_lin=0.5 * mass, kp_ang=1.0, kd_ang=0.2)
        view = sim.track_extremes()
        sim.run_resident(20, chunk=7)
        finals[name], records[name] = sim.state(), view.bodies()
        sim.close()
    assert np.isfinite(finals["scene"]).all() and (records["scene"][:, 7] > 0).all()                     # every line pulled
    assert (np.abs(finals["scene"][:, 0:3] - sc.state[:, 0:3]) > 1e-4).any(axis=1).all()
    bad = sym.differing(sym.state(m, finals["image"]), finals["scene"]) | sym.differing(sym.extremes(m, records["image"]), records["scene"])
    print(f"[ClosedLoopSim, 64 moored buoys and their mirror_y image, 20 steps in chunks of 7] {int(bad.sum())} bodies differ")
    assert not bad.any(), np.nonzero(bad)[0]


def test_closed_loop_sim_with_a_finite_depth_ensemble_and_a_sheared_current(native_built):
    """The 64 moored buoys of the test above in a depth-carrying ensemble (two members of 11 components over 25 m of water; the
    64 bodies step through the first) with the 16-knot turning profile, and the mirror_y image of all of it, both through
    ClosedLoopSim's own set_sea / set_current_profile / set_mooring: run_resident(20, chunk=7) with track_extremes leaves the
    image's final state and Extremes the images of the scene's."""
    sc, anchors, z_eq, mass = _buoys()
    k, c = Mooring.for_body(mass, sc.dt)
    depth = 25.0
    sea = SeaEnsemble([sdr.with_depth(member, depth) for member in seh.members(11, 2)], 64)
    profile = cpr.turning_profile(16, depth=depth)
    fairlead = np.array([0.05, 0.02, -0.05])
    L0 = DEPTH - 0.2                                                # taut from the first step
    m = "mirror_y"
    polar = np.asarray(sym.POLAR[m], np.float64)
    finals, records = {}, {}
    for name in ("scene", "image"):
        im = name == "image"
        scene = scenes.Scene("buoys", sym.state(m, sc.state), sym.prev(m, sc.prev), sc.params, dt=sc.dt, rho=sc.rho, g=sc.g) if im else sc
        sim = ClosedLoopSim(scene, implicit_drag=True)
        sim.set_sea(sym.sea(m, sea) if im else sea)
        sim.set_current_profile(sym.current_profile(m, profile) if im else profile)
        sim.set_mooring(anchors * polar if im else anchors, fairlead * polar if im else fairlead, length=L0, stiffness=k, damping=c)
        view = sim.track_extremes()
        sim.run_resident(20, chunk=7)
        finals[name], records[name] = sim.state(), view.bodies()
        sim.close()
    assert np.isfinite(finals["scene"]).all() and (records["scene"][:, 7] > 0).all()                     # every line pulled
    assert (np.abs(finals["scene"][:, 0:3] - sc.state[:, 0:3]) > 1e-4).any(axis=1).all()
    bad = sym.differing(sym.state(m, finals["image"]), finals["scene"]) | sym.differing(sym.extremes(m, records["image"]), records["scene"])
    print(f"[ClosedLoopSim, 64 moored buoys in a finite-depth ensemble under a sheared current and their mirror_y image, 20 steps in chunks of 7] "
          f"{int(bad.sum())} bodies differ")
    assert not bad.any(), np.nonzero(bad)[0]
