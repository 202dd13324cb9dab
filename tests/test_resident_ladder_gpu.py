"""The ladder of the resident entries (hydro_step_fused_tiled_multi_rec .. _stat): every entry takes its predecessor's argument
groups and one more, and an option that is absent is handed down the ladder as absent.  Each option in turn is present ON ITS
OWN - log, applied wrench (body frame), pose hold, sea, seabed, mooring lines, extremes, tether, two-layer net, link tensions
(of that net), a mooring spread of three layers, a sea spectrum of 9 components (set on the engine, like the sea), a statistics
record - and launched once through the first entry that takes it and once through every later entry, the later options absent: state,
prev_out, the energy pair, the log and every record the launch writes are the same bits in all of them.  A group that an entry,
a link of the launch chain or a kernel's signature dropped, transposed or handed on under another name shows here.

n = 65 (two tiles, the second with one live lane), 2 steps, f32 coefficients, explicit drag, with the kinetic energy.  Every
comparison is of bits; every call is a valid one."""
import numpy as np
import pytest
import torch

import sea_spectrum_reference as ssr
import statistics_contract as sc
from designed_populations import BED, bed_pop, hold_pop, SEA  # noqa: F401  (fixtures are requested by name)
from mooring_population import line_population
from mooring_spread_population import spread_population
from silver2_isaacsim_amd import statistics as stx
from resident_harness import _buffers, DT, _engine, ENTRIES, _ke, _log, _same_bits, step, _tiled, _watched
from tether_net_population import net_for, net_population

pytestmark = pytest.mark.gpu
N, STEPS, STEP0 = 65, 2, 3
LADDER = ("rec", "app", "ctl", "sea", "bed", "moor", "ext", "teth", "net", "peak", "spread", "irr", "stat")
# option -> the first entry that takes it
OWN = dict(log="rec", applied="app", control="ctl", sea="sea", seabed="bed", mooring="moor", extremes="ext", tether="teth", net="net", peaks="peak",
           spread="spread", spectrum="irr", statistics="stat")
WRITES = ("log", "extremes", "peaks", "statistics")               # the options that move nobody: they leave a record
SPECTRUM = ssr.truncated(ssr.designed_spectrum(), 9)
CHANNELS = (2, 5)                                                 # the statistics row: z and vz (nothing is moored in it)


@pytest.fixture(scope="module")
def pop(bed_pop):
    """The first 65 bodies of the tether net's population (the bed population: tile 0 touches the bed, body 64 does not), with
    the applied wrench, control record and mooring lines the feature modules give them."""
    _, _, params, applied, ctl = bed_pop
    st, pv, pr, net, _ = net_population()
    assert np.array_equal(pr[:N], params["f32"][:N])
    moor = line_population(st[:321], pr[:321])
    levels = sc.gap_levels(st[:N][:, [stx.STATE_FIELD[c] for c in CHANNELS]], 26)
    return dict(st=st, pv=pv, params=params["f32"], applied=applied[:N], ctl=ctl[:N], moor=moor[:N], spread=spread_population(st[:321], pr[:321], moor)[:N, 0:27],
                tether=net_for(net, N, 1), net=net_for(net, N, 2), levels=levels)


def launch(eng, entry, option, pop):
    """One launch of `entry` with `option` present and nothing else; everything it wrote: [state, prev_out, ke] and the record."""
    cur, old = _buffers(pop["st"], pop["pv"], N)
    ke = _ke()
    log = _log(STEPS, len(_watched(N))) if option == "log" else None
    if entry == "rec":
        eng.step_fused_tiled_multi_rec(cur, old, N, DT, STEPS, log, 1, 1, 0, ke_out=ke)
        torch.cuda.synchronize()
        return [old, cur[:, 7:13], ke, log]
    takes = ENTRIES[entry][1]
    layers = 2 if option in ("net", "peaks") else 1
    given = dict(applied=_tiled(pop["applied"]) if option == "applied" else None,
                 control=_tiled(pop["ctl"]) if option == "control" else None,
                 mooring=_tiled(pop["moor"]) if option == "mooring" else _tiled(pop["spread"]) if option == "spread" else None,
                 mooring_layers=3 if option == "spread" else None,
                 statistics=eng.statistics_reset(eng.alloc_statistics(N), N) if option == "statistics" else None,
                 levels=_tiled(pop["levels"]) if option == "statistics" else None, channels=CHANNELS if option == "statistics" else None,
                 extremes=eng.extremes_reset(eng.alloc_tiled(8, N), N) if option == "extremes" else None,
                 tether=_tiled(pop["tether" if option == "tether" else "net"]) if option in ("tether", "net", "peaks") else None,
                 peaks=eng.alloc_tiled(layers, N) if option == "peaks" else None)
    assert all(value is None or name in takes or (name == "channels" and "channel_a" in takes) for name, value in given.items()), (entry, option)
    state, prev = step(eng, entry, cur, old, N, STEPS, frame="body", ke=ke, log=log, step0=STEP0 if "step0" in takes else 0,
                       layers=layers if "layers" in takes else None, **given)
    torch.cuda.synchronize()
    return [state, prev, ke] + [x for x in (log, given["extremes"], given["peaks"], given["statistics"]) if x is not None]


def test_an_option_on_its_own_is_the_same_bits_through_every_later_entry(pop, native_built):
    plain = _engine(N, pop["params"], "f32")
    cur, old = _buffers(pop["st"], pop["pv"], N)
    ke = _ke()
    plain.step_fused_tiled_multi(cur, old, N, DT, STEPS, ke_out=ke)
    torch.cuda.synchronize()
    still = [old.clone(), cur[:, 7:13].clone(), ke]
    plain.close()
    nets = moored = None
    for option, own in OWN.items():
        eng = _engine(N, pop["params"], "f32")
        if option == "log":
            eng.set_watch(_watched(N))
        if option == "sea":
            eng.set_sea(SEA)
        if option == "seabed":
            eng.set_seabed(BED)
        if option == "spectrum":
            eng.set_sea_spectrum(SPECTRUM)
        entries = LADDER[LADDER.index(own):]
        runs = [launch(eng, entry, option, pop) for entry in entries]
        for entry, got in zip(entries[1:], runs[1:]):
            assert len(got) == len(runs[0]) and all(_same_bits(x, y) for x, y in zip(got, runs[0])), (option, own, entry)
        # the option is there: it moves the bodies, or it moves nothing and leaves its record
        against = nets if option == "peaks" else still            # (the link tensions come with their net: nothing feeds back)
        same = all(_same_bits(x, y) for x, y in zip(runs[0][:3], against))
        assert same == (option in WRITES), option
        if option == "log":
            assert not torch.isnan(runs[0][3]).all()
        if option == "extremes":
            assert not _same_bits(runs[0][3], eng.extremes_reset(eng.alloc_tiled(8, N), N))
        if option == "net":
            nets = runs[0]
        if option == "peaks":
            assert (runs[0][3] > 0).any()
        if option == "mooring":
            moored = runs[0]
        if option == "spread":                                    # three layers are not layer 0 alone: body 64 has a line in layer 1
            assert not all(_same_bits(x, y) for x, y in zip(runs[0][:3], moored))
        if option == "statistics":
            record = stx.unpack(runs[0][3].cpu().numpy(), N)
            assert (record["n"] == STEPS).all() and np.isfinite(record["sums"]).all() and (record["sums"] != 0).all()
        eng.close()
