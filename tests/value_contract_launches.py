"""The launches tests/test_value_contract_gpu.py and tests/test_parameter_contract_gpu.py share: the population and engines
fixtures (the bodies, net and mooring lines of tests/test_tether_net_gpu.py, and the same with the exact-zero bodies), one caller
per open-loop entry (`OPEN_LOOP`), `_isolated` (clean, poisoned, clean again) and `_everything` (one resident launch with every
option on, through `peak` or any earlier entry, or through `spread`, `irr` and `stat`: the five kernel families above _peak).  Nothing is asserted here but what those two modules ask through these callers."""
import numpy as np
import pytest
import torch

import mooring_population as mp
import statistics_contract as sc
import value_contract as vc
from mooring_spread_population import spread_population
from silver2_isaacsim_amd import extremes as ex
from silver2_isaacsim_amd import statistics as stx
from silver2_isaacsim_amd.sea import SeaState
from designed_populations import BED, SEA
from resident_harness import _buffers, DEV, DT, _engine, _from, _ke, _log, NAN, _rows, step, _tiled
from tether_net_population import net_population

SIZES, STEPS = vc.SIZES, vc.STEPS
TIME = 0.75                                                       # the open-loop sea entries' time (s)
STEP0 = 3
CURRENT = SeaState((0.5, -0.2, 0.05))                             # a sea without waves: the wrench does not depend on x and y


@pytest.fixture(scope="module")
def pop(bed_pop, hold_pop):
    """The bodies, net and mooring lines of tests/test_tether_net_gpu.py (the first 321), and the same with the exact-zero bodies."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, groups = net_population()
    n = max(SIZES)
    assert np.array_equal(pr[:n], params["f32"][:n])
    moor = mp.line_population(st[:n], params["f32"][:n])
    base = dict(st=st[:n], pv=pv[:n], applied=applied[:n], ctl=ctl[:n], moor=moor)
    zst, zpv, zapplied, zctl, zmoor = vc.exact_zero_bodies(*base.values())
    pulling = np.flatnonzero(mp.population_report(moor, st[:n])[0] & mp.OFF_TIES)
    return dict(base, params={k: v[:n] for k, v in params.items()}, net=net, rec=net[:, 0:7], groups=groups, pulling=pulling,
                spread=spread_population(st[:n], params["f32"][:n], moor),
                zero=dict(st=zst, pv=zpv, applied=zapplied, ctl=zctl, moor=zmoor), hold=(hold_pop[0][:n], hold_pop[1][:n], hold_pop[5]))


@pytest.fixture(scope="module")
def engines(pop, native_built):
    """engines(n, coeff, semantics): the module's one engine of that size and coefficient format, back at its defaults."""
    made = {}

    def get(n, coeff, semantics="numba"):
        if (n, coeff) not in made:
            made[n, coeff] = _engine(n, pop["params"][coeff], coeff)
        eng = made[n, coeff]
        eng.set_tuning()
        eng.set_semantics(semantics)
        eng.set_sea_spectrum(None)
        eng.set_sea(None)
        eng.set_seabed(None)
        eng.set_watch(None)
        return eng
    yield get
    for eng in made.values():
        eng.close()


def _soa(a):
    """(n, F) host -> (F, n) device."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _host(t):
    return t.cpu().numpy()


def _aos(st):
    return _dev(st[:, 0:3]), _dev(st[:, [6, 3, 4, 5]]), _dev(st[:, 3:7]), _dev(st[:, 7:13])


def _wrench_own(eng, st, pv, n):
    eng.set_prev_velocity(pv)
    return [_host(eng.step_wrench(_soa(st), DT)).T]


def _wrench_ext(eng, st, pv, n):
    return [_host(eng.step_wrench(_soa(st), DT, prev=_soa(pv))).T]


def _wrench_tiled(eng, st, pv, n):
    return [_from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv)), n)]


def _wrench_tiled_ke(eng, st, pv, n):
    return [_from(eng.step_wrench_tiled(_tiled(st), n, DT, prev=_tiled(pv), ke_out=_ke()), n)]      # (the wrench only: the energy is a sum)


def _wrench_tiled_sea(eng, st, pv, n):
    eng.set_sea(SEA)
    out = _from(eng.step_wrench_tiled_sea(_tiled(st), n, DT, TIME, prev=_tiled(pv)), n)
    eng.set_sea(None)
    return [out]


def _wrench_aos(eng, st, pv, n, xyzw=False, sea=False):
    pos, wxyz, xyzw_q, vel = _aos(st)
    eng.set_prev_velocity(pv)
    if sea:
        eng.set_sea(SEA)
        F, T = eng.step_wrench_aos_sea(pos, xyzw_q if xyzw else wxyz, vel, DT, TIME, quat_xyzw=xyzw)
        eng.set_sea(None)
    else:
        F, T = eng.step_wrench_aos(pos, xyzw_q if xyzw else wxyz, vel, DT, quat_xyzw=xyzw)
    return [_host(F), _host(T)]


def _accel(st, pv):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((st[:, 7:13] - pv) / np.float32(DT)).astype(np.float32)


def _components(eng, st, pv, n):
    out, ratio = eng.step_components(_soa(st), _soa(_accel(st, pv)))
    return [_host(out).T, _host(ratio)[:, None]]


def _components_aos(eng, st, pv, n):
    a = _accel(st, pv)
    out, ratio = torch.full((8, n, 3), NAN, dtype=torch.float32, device=DEV), torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    eng.step_components_aos(_dev(st[:, 0:3]), _dev(st[:, 3:7]), _dev(st[:, 7:10]), _dev(st[:, 10:13]), _dev(a[:, 0:3]), _dev(a[:, 3:6]), out, ratio)
    return [_host(out).transpose(1, 0, 2).reshape(n, 24), _host(ratio)[:, None]]


OPEN_LOOP = {
    "step_wrench, engine-owned previous velocity": _wrench_own,
    "step_wrench, caller-owned previous velocity": _wrench_ext,
    "step_wrench_tiled": _wrench_tiled,
    "step_wrench_tiled_ke": _wrench_tiled_ke,
    "step_wrench_tiled_sea": _wrench_tiled_sea,
    "step_wrench_aos wxyz": _wrench_aos,
    "step_wrench_aos xyzw": lambda *a: _wrench_aos(*a, xyzw=True),
    "step_wrench_aos_sea": lambda *a: _wrench_aos(*a, sea=True),
    "step_components": _components,
    "step_components_aos": _components_aos,
}


def _isolated(run, clean, poisoned, bodies, what):
    """run(state, prev) -> list of (n, F) arrays: clean, poisoned, clean again.  The poisoned launch leaves every other body the
    clean bits, and the clean launch afterwards is the clean launch.  Returns (the clean outputs, the poisoned ones)."""
    want = run(*clean)
    got = run(*poisoned)
    again = run(*clean)
    for i, (g, w, a) in enumerate(zip(got, want, again)):
        vc.assert_isolated(g, w, bodies, what + (i,))
        vc.assert_same_bits(a, w, what + (i, "the clean launch afterwards"))
    return want, got


STAT_CHANNELS = (2, 6)                                            # `_everything`'s statistics: z and the tension


def _words(record, n):
    """The statistics record's 11 words per body, (n, 11) as float32 BIT PATTERNS: value_contract's checkers compare bits."""
    rec = stx.unpack(record.cpu().numpy(), n)
    return np.concatenate([rec["sums"].view(np.uint32), rec["up"], rec["n"][:, None]], axis=1).view(np.float32)


def _everything(eng, pop, n, steps, implicit, *, st, pv, ctl, net, moor=None, seed=None, ke=False, entry="peak", layers=4, applied=True, chunks=None, bed=BED, sea=SEA,
                spectrum=None):
    """One resident launch (or `chunks` of them) with everything on: sea, bed, pose hold, a body-frame applied wrench, mooring,
    extremes (from `seed`, default the empty record), the net with peaks, the recorder on every body.  `entry` "spread", "irr" and
    "stat" take all of it with the designed spread of three layers in place of the single line; `spectrum` (a SeaSpectrum) takes the
    place of `sea` for "irr" and "stat" - the _irr and _irr_stat kernel families -; "stat" keeps a statistics record of STAT_CHANNELS
    from the empty record against gap levels of the CLEAN population's initial z (the same levels whatever `st` holds).  Returns
    per-body arrays: state (n, 13), prev_out (n, 6), log (n, steps * 19), extremes (n, 8), peaks (n, layers), statistics (n, 11 words;
    (n, 0) where the entry keeps none), and the rows (steps, n, 19)."""
    assert spectrum is None or entry in ("irr", "stat"), entry
    eng.set_sea_spectrum(None)
    eng.set_sea(None if spectrum is not None else sea)
    eng.set_sea_spectrum(spectrum)
    eng.set_seabed(bed)
    eng.set_watch(list(range(n)))
    cur, old = _buffers(st, pv, n)
    takes = {"moor": 0, "ext": 1, "teth": 2, "net": 3, "peak": 4, "spread": 5, "irr": 5, "stat": 6}[entry]
    kw = dict(mooring=_tiled((pop["moor"] if moor is None else moor)[:n]), control=_tiled(ctl[:n]) if ctl is not None else None, applied=_tiled(pop["applied"][:n]) if applied else None, frame="body")
    record = peaks = statistics = None
    if takes >= 5:
        kw.update(mooring=_tiled((pop["spread"][:, 0:27] if moor is None else moor)[:n]), mooring_layers=3)
    if takes >= 6:
        statistics = eng.statistics_reset(eng.alloc_statistics(n), n)
        levels = sc.gap_levels(np.stack([pop["st"][:n, 2], np.zeros(n, np.float32)], axis=1), 27)
        kw.update(statistics=statistics, levels=_tiled(levels), channels=STAT_CHANNELS)
    if takes >= 1:
        record = kw["extremes"] = _tiled(ex.Extremes.empty(n) if seed is None else seed)
    if takes >= 2:
        kw["tether"] = _tiled(net[:n, :7 * (layers if takes >= 3 else 1)])
    if takes >= 3:
        kw["layers"] = layers
    if takes >= 4:
        peaks = kw["peaks"] = eng.alloc_tiled(layers, n)
    logs, done = [], 0
    for k in chunks or [steps]:
        log = _log(k, n)
        step(eng, entry, cur, old, n, k, step0=STEP0 + done, implicit=implicit, ke=_ke() if ke else None, log=log, **kw)
        cur, old = old, cur
        logs.append(_rows(log))
        done += k
    torch.cuda.synchronize()
    rows = np.concatenate(logs)
    out = dict(state=_from(cur, n), prev=_from(old, n)[:, 7:13], log=rows.transpose(1, 0, 2).reshape(n, -1), rows=rows)
    if record is not None:
        out["extremes"] = _from(record, n)
    if peaks is not None:
        out["peaks"] = _from(peaks, n)
    out["statistics"] = _words(statistics, n) if statistics is not None else np.zeros((n, 0), np.float32)
    eng.set_sea_spectrum(None)
    return out


PER_BODY = ("state", "prev", "log", "extremes", "peaks", "statistics")
