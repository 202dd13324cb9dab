"""The population of the symmetry tests' later rungs (tether, net, link tensions, spread, irregular sea), built without a device:
shared by tests/test_symmetry.py, which asserts what it is made of, and tests/test_symmetry_gpu.py, which runs it.

It is the population of tests/test_mooring_spread_gpu.py - the first 321 bodies of tether_net_population.net_population with
mooring_population.line_population and mooring_spread_population.spread_population over them - RESEATED: designed_populations.
tilted_boxes moves four bodies in five, in z only, onto ONE corner, because the bed's corner sum is the one order-sensitive sum on
the device (tests/test_symmetry_gpu.py) and 59 % of the population as drawn stands on two or more corners.  The mooring lines and
the spread are drawn anew from the moved states (every anchored line is built from its own body's state; the ties at bodies
0 .. 7 are not moved and keep their records); the controller's targets follow the bodies in z.  The tether net is NOT drawn anew:
its lines join two bodies, and the moved population keeps enough of them pulling (asserted in tests/test_symmetry.py).
"""
import numpy as np

from designed_populations import tilted_boxes
from mooring_population import line_population
from mooring_spread_population import spread_population
from tether_net_population import net_for, net_population

N = 321
NET_LAYERS = 2                                                    # the layers of the net the resident tests run
SPREAD_LAYERS = 3                                                 # "the spread of three": layer 3 of the designed spread is zeros


def reseated_population():
    """dict(st, drawn (the states before reseating), pv, params {f32, f16}, net (322, 28), spread (321, 36), lines (321, 9), groups):
    see the module's docstring.  The applied wrench and the control record are the fixtures' (designed_populations.bed_pop); the
    caller moves the targets with `follow`."""
    st, pv, pr, net, groups = net_population()
    st, pv, pr = st[:N], pv[:N], pr[:N]
    moved, _, _ = tilted_boxes(st, pv, pr)
    rec = line_population(st, pr)
    changed = moved[:, 2] != st[:, 2]
    lines = np.where(changed[:, None], line_population(moved, pr), rec)
    spread = spread_population(moved, pr, lines)
    p16 = pr.copy()
    p16[:, 3:10] = pr[:, 3:10].astype(np.float16).astype(np.float32)
    return dict(st=moved, drawn=st, pv=pv, params={"f32": pr, "f16": p16}, net=net, spread=spread, lines=lines, groups=groups)


def follow(ctl, drawn, moved):
    """The control record with its targets moved in z as the bodies were, so that the law's terms keep their sizes."""
    out = ctl.copy()
    out[:, 2] = (ctl[:, 2].astype(np.float64) + (moved[:, 2].astype(np.float64) - drawn[:, 2])).astype(np.float32)
    return out


def net_of(pop, n, layers=NET_LAYERS):
    """The net of the first n bodies: tether_net_population.net_for."""
    return net_for(pop["net"], n, layers)
