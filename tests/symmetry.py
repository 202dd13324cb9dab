"""The three maps under which the model is EXACTLY symmetric, and the predicate the symmetry tests share
(tests/test_symmetry.py, tests/test_symmetry_gpu.py; DESIGN.md, "Sign symmetry").

The water surface, gravity and the bed are horizontal, so a mirror in the plane y = 0, a mirror in x = 0 and their product,
a half turn about z, map a scene onto an equally valid one.  Each of them only changes signs of inputs, and IEEE arithmetic
is exactly odd - fl(-a) = -fl(a), fma(-a, b, -c) = -fma(a, b, c) - so an evaluation in which every term of every sum has the
same parity returns the same bits with the predicted signs.  The table, stated once:

    map         polar vector    axial vector    quaternion (x, y, z, w)
    mirror_y    (+, -, +)       (-, +, -)       (-, +, -, +)
    mirror_x    (-, +, +)       (+, -, -)       (+, -, -, +)
    half_turn   (-, -, +)       (-, -, +)       (-, -, +, +)

polar: positions, linear velocities, forces, anchors, fairleads, the current, the wave vector, centres; axial: angular
velocities and torques; a mirrored body's frame is the mirrored frame, so body-frame records transform like world-frame
ones.  Scalars (dimensions, coefficients, mass, gains, limits, lengths, the bed's constants, amplitudes, frequencies,
phases, eta, the submersion ratio, energies, tensions) do not change.  An extremes record swaps min and max of a flipped
axis: min' = -max, max' = -min.

The records of the later rungs, stated once like the rest:

    record              shape       image
    tether              (n, 7)      [b | L0 | k | c | partner]: the fairlead b (body frame) is polar; L0, k, c keep their values
                                    and so does the partner LANE - the maps do not renumber bodies
    net                 (n, 7 L)    a tether record per layer, each mapped as `tether`
    spread              (n, 9 L)    a mooring record per layer, each mapped as `mooring`
    link tensions       (n, L)      scalars: the same bits (and so is tension_max of the extremes record)
    sea                 -           `sea()` serves every kind of sea, sea.SeaState, sea.SeaSpectrum and sea.SeaEnsemble (it builds
                                    type(s)): the current and every component's (kx, ky) are polar, amplitude, omega and phase
                                    scalars - and so is a spectrum's DEPTH, which the image carries
    sea ensemble        -           member by member, the member ORDER and bodies_per_sea unchanged: block m of the bodies steps
                                    through the image of member m - the maps do not renumber bodies
    current profile     -           `current_profile()`: the knots' z_l are scalars, the V_l polar (so V_0 and every slope D_l
                                    change sign only)
    levels              (n, 2)      `levels()`: the level of a channel the map flips changes sign, L' = -L; the others keep theirs
    statistics          dict        `statistics()`: sums (n, 4) [S1_a S2_a S1_b S2_b], up (n, 2), n (n,).  A channel the map does not
                                    flip - z, vz and tension always, and whichever of x, y, vx, vy the map leaves alone - keeps
                                    every word.  A flipped channel, against L' = -L: d' = -d exactly, so S1' = -S1 and S2 keeps
                                    its bits.  n keeps its bits.  THE UP-CROSSING WORD OF A FLIPPED CHANNEL IS NOT COMPARABLE: an
                                    up-crossing of L by x is a DOWN-crossing of -L by -x, and the record counts no down-crossings.
                                    That one word, of that slot only, is left out (`statistics_left_out`); `statistics()` puts 0
                                    in its place

The sums the later rungs add - over a net's or a spread's layers, over a spectrum's components, over a profile's knots, over
the steps of a statistics record - run in an order the maps do not permute (unlike the bed's corners), so they keep the
predicate without a tolerance.

One function per record kind; each returns the IMAGE of a record (the maps are involutions: the image of the image is the
record).  `equal` is the predicate: float equality with NaN == NaN, so -0 == +0 (a dry body returns +0 and the image of +0
is -0) - no tolerance.
"""
import numpy as np

MAPS = ("mirror_y", "mirror_x", "half_turn")
POLAR = {"mirror_y": (1, -1, 1), "mirror_x": (-1, 1, 1), "half_turn": (-1, -1, 1)}
AXIAL = {"mirror_y": (-1, 1, -1), "mirror_x": (1, -1, -1), "half_turn": (-1, -1, 1)}
QUAT = {"mirror_y": (-1, 1, -1, 1), "mirror_x": (1, -1, -1, 1), "half_turn": (-1, -1, 1, 1)}
SAME3 = (1, 1, 1)
# the bed's corner i has the signs of (i & 1, i & 2, i & 4) along the body's x, y, z: the image of corner i is corner i ^ this
CORNER_XOR = {"mirror_y": 2, "mirror_x": 1, "half_turn": 3}
# the components of hydro_step_components, in the reference's order: buoyancy F, drag F, lift F, drag T, added-mass F,
# added-mass T, centre of buoyancy, centre of pressure
COMPONENT_KINDS = (POLAR, POLAR, POLAR, AXIAL, POLAR, AXIAL, POLAR, POLAR)


def _times(x, signs):
    x = np.asarray(x)
    return x * np.asarray(signs, dtype=x.dtype)


def state(g, s):
    """(n, 13) [p | q xyzw | v | omega]."""
    return _times(s, POLAR[g] + QUAT[g] + POLAR[g] + AXIAL[g])


def prev(g, pv):
    """(n, 6) previous velocity [v | omega]."""
    return _times(pv, POLAR[g] + AXIAL[g])


def wrench(g, w):
    """(n, 6) [F | T], world frame."""
    return _times(w, POLAR[g] + AXIAL[g])


def applied(g, a):
    """(n, 6) applied [F | T], in either frame: the mirrored body's frame is the mirrored frame."""
    return wrench(g, a)


def control(g, c):
    """(n, 17) pose-hold record [p* | q* | kp_lin(3) | kd_lin(3) | kp_ang | kd_ang | f_max | t_max]."""
    return _times(c, POLAR[g] + QUAT[g] + (1,) * 10)


def mooring(g, m):
    """(n, 9) line record [anchor (world) | fairlead (body) | L0 | k | c]."""
    return _times(m, POLAR[g] + POLAR[g] + SAME3)


def tether(g, rec):
    """(n, 7) tether record [fairlead b (body) | L0 | k | c | partner lane]: b is polar, the rest - the partner included - unchanged."""
    return _times(rec, POLAR[g] + (1, 1, 1, 1))


def net(g, rec):
    """(n, 7 L) tether net: `tether`, layer by layer."""
    rec = np.asarray(rec)
    assert rec.ndim == 2 and rec.shape[1] % 7 == 0, rec.shape
    return np.concatenate([tether(g, rec[:, 7 * l:7 * l + 7]) for l in range(rec.shape[1] // 7)], axis=1)


def spread(g, rec):
    """(n, 9 L) mooring spread: `mooring`, layer by layer."""
    rec = np.asarray(rec)
    assert rec.ndim == 2 and rec.shape[1] % 9 == 0, rec.shape
    return np.concatenate([mooring(g, rec[:, 9 * l:9 * l + 9]) for l in range(rec.shape[1] // 9)], axis=1)


def extremes(g, e):
    """(n, 8) [x_min x_max | y_min y_max | z_min z_max | speed2_max | tension_max]: a flipped axis swaps its pair."""
    e = np.asarray(e)
    out = e.copy()
    for a, sign in enumerate(POLAR[g]):
        if sign < 0:
            out[:, 2 * a], out[:, 2 * a + 1] = -e[:, 2 * a + 1], -e[:, 2 * a]
    return out


def sea(g, s):
    """A sea.SeaState, a sea.SeaSpectrum or a sea.SeaEnsemble (the image is of the same kind): the current and the wave vector
    (kx, ky) are polar - never a heading angle; a spectrum's depth is a scalar and the image has it; an ensemble maps member by
    member, in the members' order, over the same bodies_per_sea."""
    if hasattr(s, "members"):
        return type(s)([sea(g, member) for member in s.members], s.bodies_per_sea)
    sx, sy, sz = POLAR[g]
    current = (sx * s.current[0], sy * s.current[1], sz * s.current[2])
    out = type(s)(current, s.depth) if hasattr(s, "depth") else type(s)(current)
    for a, kx, ky, om, ph in s.waves:
        out.add_wave(a, sx * kx, sy * ky, om, ph)
    return out


def current_profile(g, p):
    """A sea.CurrentProfile: the knots' z_l are scalars, the V_l polar."""
    return type(p)(p.z, _times(p.v, POLAR[g]))


def flips(g, channel):
    """Whether the map changes the sign of a statistics channel (0 .. 6: x, y, z, vx, vy, vz, tension)."""
    return channel < 6 and POLAR[g][channel % 3] < 0


def levels(g, lev, channels):
    """(n, 2) reference levels of the two channel slots: the level of a flipped channel changes sign."""
    return _times(lev, tuple(-1 if flips(g, c) else 1 for c in channels))


def statistics(g, rec, channels):
    """The statistics record as statistics.unpack gives it - sums (n, 4), up (n, 2), n (n,) - taken against `levels()`: a flipped
    slot's S1 changes sign and its S2 keeps its bits; its up-crossing word is NOT predicted (an up-crossing of L by x is a
    down-crossing of -L by -x) and 0 stands in its place: compare through `statistics_words` and `statistics_left_out`."""
    sums, up = np.array(rec["sums"], np.float64, copy=True), np.array(rec["up"], np.uint32, copy=True)
    for slot, c in enumerate(channels):
        if flips(g, c):
            sums[:, 2 * slot] = -sums[:, 2 * slot]
            up[:, slot] = 0
    return {"sums": sums, "up": up, "n": np.array(rec["n"], np.uint32, copy=True)}


def statistics_words(rec):
    """(n, 7) float64 [S1_a S2_a S1_b S2_b | up_a up_b | n] of a statistics record (a uint32 is exact in a double)."""
    return np.concatenate([np.asarray(rec["sums"], np.float64), np.asarray(rec["up"], np.float64), np.asarray(rec["n"], np.float64)[:, None]], axis=1)


def statistics_left_out(g, channels):
    """The columns of `statistics_words` that are not comparable under g: the up-crossing word of each flipped slot."""
    return [4 + slot for slot, c in enumerate(channels) if flips(g, c)]


def statistics_differing(g, got, want, channels):
    """(n,) bool: the bodies on which the record `got` of the image, mapped back by `statistics`, differs from the scene's `want` -
    the up-crossing word of a flipped slot left out on both sides."""
    a, b = statistics_words(got), statistics_words(want)
    cols = statistics_left_out(g, channels)
    a[:, cols], b[:, cols] = 0.0, 0.0
    return differing(a, b)


def sea_sample(g, w):
    """(n, 4) [eta | u] of hydro_sea_sample and hydro_sea_spectrum_sample."""
    return _times(w, (1,) + POLAR[g])


def components(g, c):
    """(n, 8, 3) in the order of COMPONENT_KINDS."""
    return _times(c, np.array([kind[g] for kind in COMPONENT_KINDS]))


def log_row(g, row):
    """(..., n, 19) recorded rows: the state, then the wrench that produced it."""
    return _times(row, POLAR[g] + QUAT[g] + POLAR[g] + AXIAL[g] + POLAR[g] + AXIAL[g])


def equal(a, b):
    """Equal under g: the image computed equals the image predicted, by float equality (a NaN equals a NaN)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def differing(a, b):
    """(n,) bool: the bodies (leading axis) on which `equal` fails."""
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return ~same.reshape(len(a), -1).all(axis=1)
