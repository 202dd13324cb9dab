"""ctypes binding of libhydro.so (the C ABI declared in include/hydro.h).

The shared library is built in-tree by `silver2_isaacsim_amd.build.build()`
(`__graft_entry__.build()` calls it) into `silver2_isaacsim_amd/lib/`.  There is
no CPU fallback: if the library is missing or fails to load, importing the
binding raises, and every product entry point needs it.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhydro.so")

STATE_FIELDS, PREV_FIELDS, PARAM_FIELDS, WRENCH_FIELDS, COMP_FIELDS = 13, 6, 11, 6, 24
CTL_FIELDS = 17                         # the control record of hydro_step_fused_tiled_multi_ctl
MOOR_FIELDS = 9                         # the mooring record of hydro_step_fused_tiled_multi_moor: a(3) | b(3) | L0 | k | c
EXT_FIELDS = 8                          # the extremes record of hydro_step_fused_tiled_multi_ext: x, y, z min max | speed2_max | tension_max
TETH_FIELDS = 7                         # the tether record of hydro_step_fused_tiled_multi_teth: b(3) | L0 | k | c | partner lane
TETH_LAYERS_MAX = 4                     # layers of tether records in the net of hydro_step_fused_tiled_multi_net
MOOR_LAYERS_MAX = 4                     # layers of mooring records in the spread of hydro_step_fused_tiled_multi_spread
TILE = 64
BATCH_MAX = 32
WATCH_MAX = 65536
SEA_WAVES_MAX = 8                       # regular wave components of a sea state (hydro_set_sea)
SEA_FIELDS = 4                          # the record of hydro_sea_sample: eta, u_x, u_y, u_z
SPECTRUM_WAVES_MAX = 64                 # wave components of a sea spectrum (hydro_set_sea_spectrum)
SEA_ENSEMBLE_MAX = 1024                 # members of a sea ensemble (hydro_set_sea_ensemble)
CURRENT_KNOTS_MAX = 16                  # knots of a current profile (hydro_set_current_profile)
# the statistics record of hydro_step_fused_tiled_multi_stat: channels, and the record in 4-byte units per body (4 doubles + 3 words)
STAT_X, STAT_Y, STAT_Z, STAT_VX, STAT_VY, STAT_VZ, STAT_TENSION = range(7)
STAT_CHANNELS = 7
STAT_BYTES_PER_BODY = 44
STAT_FIELDS = STAT_BYTES_PER_BODY // 4  # the record as a tiled buffer of 4-byte fields: (tiles, 11, 64) = 2 816 B per tile
STAT_LEVEL_FIELDS = 2                   # the level record: one level per body and channel slot


class Scene(ctypes.Structure):
    """hydro_scene_t (include/hydro.h): one scene of a hydro_step_wrench_tiled_batch launch."""
    _fields_ = [("engine", c_void_p), ("n", c_int64),
                ("state", c_void_p), ("state_tile_stride", c_int64),
                ("prev", c_void_p), ("prev_tile_stride", c_int64),
                ("wrench", c_void_p), ("wrench_tile_stride", c_int64)]


class SeaWave(ctypes.Structure):
    """hydro_sea_wave_t (include/hydro.h): one regular wave component."""
    _fields_ = [("amplitude", c_double), ("kx", c_double), ("ky", c_double), ("omega", c_double), ("phase", c_double)]


class Sea(ctypes.Structure):
    """hydro_sea_t (include/hydro.h): the sea state hydro_set_sea takes."""
    _fields_ = [("current", c_double * 3), ("waves", c_int), ("wave", SeaWave * SEA_WAVES_MAX)]


class SeaSpectrum(ctypes.Structure):
    """hydro_sea_spectrum_t (include/hydro.h): the irregular sea hydro_set_sea_spectrum takes; `wave` points at `waves` SeaWave."""
    _fields_ = [("current", c_double * 3), ("waves", c_int), ("wave", POINTER(SeaWave))]


class CurrentProfile(ctypes.Structure):
    """hydro_current_profile_t (include/hydro.h): the sheared current hydro_set_current_profile takes; `z` points at `knots`
    floats, `v` at `knots` x 3."""
    _fields_ = [("knots", c_int), ("z", POINTER(ctypes.c_float)), ("v", POINTER(ctypes.c_float))]


class Seabed(ctypes.Structure):
    """hydro_seabed_t (include/hydro.h): the plane and the five mass-normalised contact constants hydro_set_seabed takes."""
    _fields_ = [("z", c_double), ("stiffness", c_double), ("damping", c_double), ("friction", c_double),
                ("slip_speed", c_double), ("friction_rate", c_double)]


HYDRO_OK, HYDRO_E_ARG, HYDRO_E_ALLOC, HYDRO_E_LAUNCH, HYDRO_E_DEVICE, HYDRO_E_STATE = 0, -1, -2, -3, -4, -5
HYDRO_SEM_NUMBA, HYDRO_SEM_WARP = 0, 1
HYDRO_FRAME_WORLD, HYDRO_FRAME_BODY = 0, 1          # frame of an applied wrench (hydro_step_fused_tiled_multi_app)
STATUS_NAMES = {v: k for k, v in list(globals().items()) if k == "HYDRO_OK" or k.startswith("HYDRO_E_")}

# every symbol include/hydro.h declares: (restype, argtypes)
_FP = POINTER(c_void_p)      # table of field pointers (const float *const [N])
# The argument groups of the hydro_step_fused_tiled_multi* entries, each stated once, in the header's order within a group:
# an entry is the base group, the groups of the options it takes, `step0` from the _sea entry on, and the stream.
_MULTI = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double, c_int,       # h, n, state, prev (+ strides), dt, steps
          c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p]                   # state_out, prev_out (+ strides), implicit_drag, rotational, ke_out_dev
_REC = [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int64, POINTER(c_int64)]       # log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host
_APP = [c_void_p, c_int64, c_int]                                                         # applied, applied_tile_stride, applied_frame
_CTL = _MOOR = _EXT = _TETH = _PEAK = [c_void_p, c_int64]                                 # a per-body record and its tile stride
_LAYERS = _STEP0 = [c_int64]                                                              # tether_layers; step0
_SPREAD = _MOOR + [c_int64]                                                               # the mooring record as a spread: + mooring_layers
_STAT = [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int]                              # statistics, levels (+ strides), channel_a, channel_b
_STREAM = [c_void_p]
_SET_FD = [c_void_p, POINTER(SeaSpectrum), c_int64, c_int64, c_double]                       # h, members, count, bodies_per_sea, depth
_SAMPLE = [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_double, c_void_p, c_int64, c_void_p]   # h, n, state (+ stride), step_index, dt, out (+ stride), stream


def _multi(*groups):
    return c_int, sum(groups, _MULTI) + _STREAM


SIGNATURES = {
    "hydro_version": (c_int, []),
    "hydro_status_string": (c_char_p, [c_int]),
    "hydro_device_count": (c_int, [POINTER(c_int)]),
    "hydro_create": (c_int, [c_int, c_int64, POINTER(c_void_p)]),
    "hydro_destroy": (c_int, [c_void_p]),
    "hydro_last_error": (c_char_p, [c_void_p]),
    "hydro_capacity": (c_int64, [c_void_p]),
    "hydro_set_scene": (c_int, [c_void_p, c_double, c_double]),
    "hydro_set_semantics": (c_int, [c_void_p, c_int]),
    "hydro_set_params_f32": (c_int, [c_void_p, c_int64, _FP, c_int]),
    "hydro_set_params_f16": (c_int, [c_void_p, c_int64, _FP, c_int]),
    "hydro_reset_prev_velocity": (c_int, [c_void_p]),
    "hydro_get_prev_velocity": (c_int, [c_void_p, c_int64, _FP, c_int]),
    "hydro_set_prev_velocity": (c_int, [c_void_p, c_int64, _FP, c_int]),
    "hydro_step_wrench": (c_int, [c_void_p, c_int64, _FP, c_double, _FP, c_void_p]),
    "hydro_step_wrench_ext": (c_int, [c_void_p, c_int64, _FP, _FP, c_double, _FP, c_void_p]),
    "hydro_step_wrench_tiled": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                        c_void_p, c_int64, c_void_p]),
    "hydro_step_wrench_tiled_batch": (c_int, [c_int, POINTER(Scene), c_double, c_void_p]),
    "hydro_step_wrench_tiled_ke": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                           c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "hydro_step_fused_tiled": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                       c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p]),
    "hydro_step_fused_tiled_ke": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                          c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "hydro_step_fused_tiled_multi": _multi(),
    "hydro_set_watch": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "hydro_watch_count": (c_int64, [c_void_p]),
    "hydro_step_fused_tiled_multi_rec": _multi(_REC),
    "hydro_step_fused_tiled_multi_app": _multi(_REC, _APP),
    "hydro_step_fused_tiled_multi_ctl": _multi(_REC, _APP, _CTL),
    "hydro_set_sea": (c_int, [c_void_p, POINTER(Sea)]),
    "hydro_sea_sample": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_double, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_sea": _multi(_REC, _APP, _CTL, _STEP0),
    "hydro_step_wrench_tiled_sea": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                            c_void_p, c_int64, c_double, c_void_p]),
    "hydro_step_wrench_aos_sea": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_double,
                                          c_void_p, c_void_p, c_double, c_void_p]),
    "hydro_step_wrench_tiled_irr": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                            c_void_p, c_int64, c_double, c_void_p]),
    "hydro_step_wrench_aos_irr": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_double,
                                          c_void_p, c_void_p, c_double, c_void_p]),
    "hydro_set_seabed": (c_int, [c_void_p, POINTER(Seabed)]),
    "hydro_seabed_wrench": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_bed": _multi(_REC, _APP, _CTL, _STEP0),
    "hydro_mooring_wrench": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_moor": _multi(_REC, _APP, _CTL, _MOOR, _STEP0),
    "hydro_extremes_reset": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_ext": _multi(_REC, _APP, _CTL, _MOOR, _EXT, _STEP0),
    "hydro_tether_wrench": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_teth": _multi(_REC, _APP, _CTL, _MOOR, _EXT, _TETH, _STEP0),
    "hydro_step_fused_tiled_multi_net": _multi(_REC, _APP, _CTL, _MOOR, _EXT, _TETH, _LAYERS, _STEP0),
    "hydro_step_fused_tiled_multi_peak": _multi(_REC, _APP, _CTL, _MOOR, _EXT, _TETH, _LAYERS, _PEAK, _STEP0),
    "hydro_step_fused_tiled_multi_spread": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STEP0),
    "hydro_set_sea_spectrum": (c_int, [c_void_p, POINTER(SeaSpectrum)]),
    "hydro_sea_spectrum_sample": (c_int, _SAMPLE),
    "hydro_step_fused_tiled_multi_irr": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STEP0),
    "hydro_statistics_reset": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hydro_step_fused_tiled_multi_stat": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STAT, _STEP0),
    "hydro_set_sea_ensemble": (c_int, [c_void_p, POINTER(SeaSpectrum), c_int64, c_int64]),
    "hydro_sea_ensemble_sample": (c_int, _SAMPLE),
    "hydro_step_fused_tiled_multi_ens": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STAT, _STEP0),
    "hydro_set_sea_finite_depth": (c_int, _SET_FD),
    "hydro_sea_finite_depth_sample": (c_int, _SAMPLE),
    "hydro_step_fused_tiled_multi_fd": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STAT, _STEP0),
    "hydro_set_current_profile": (c_int, [c_void_p, POINTER(CurrentProfile)]),
    "hydro_current_profile_sample": (c_int, _SAMPLE),
    "hydro_step_fused_tiled_multi_shear": _multi(_REC, _APP, _CTL, _SPREAD, _EXT, _TETH, _LAYERS, _PEAK, _STAT, _STEP0),
    "hydro_reserve_soa": (c_int, [c_void_p]),
    "hydro_integrate_tiled": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                      c_void_p, c_int64, c_void_p]),
    "hydro_pack_state_aos": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "hydro_unpack_wrench_aos": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "hydro_repack": (c_int, [c_void_p, c_int64, c_int, _FP, c_void_p, c_int64, c_int, c_void_p]),
    "hydro_step_wrench_aos": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_double,
                                      c_void_p, c_void_p, c_void_p]),
    "hydro_step_components": (c_int, [c_void_p, c_int64, _FP, _FP, _FP, c_void_p, c_void_p]),
    "hydro_step_components_aos": (c_int, [c_void_p, c_int64] + [c_void_p] * 6 + [_FP, c_void_p, c_void_p]),
    "hydro_kinetic_energy": (c_int, [c_void_p, c_int64, _FP, c_int, c_void_p, c_void_p]),
    "hydro_kinetic_energy_tiled": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "hydro_ke_allreduce": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "hydro_bind_rccl": (c_int, [c_void_p, c_void_p]),
    "hydro_rccl_origin": (c_char_p, []),
    "hydro_ke_rearm": (c_int, [c_void_p, c_void_p]),
    "hydro_debug_ke_fault": (c_int, [c_void_p, c_int, ctypes.c_uint32, c_int]),
    "hydro_integrate": (c_int, [c_void_p, c_int64, _FP, _FP, c_double, _FP, c_void_p]),
    "hydro_set_tuning": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "hydro_sync": (c_int, [c_void_p]),
    "hydro_stream": (c_void_p, [c_void_p]),
}

_lib = None


class HydroError(RuntimeError):
    """Non-zero status from libhydro.  A RuntimeError on purpose: the reference plugin's
    state-fetch guard treats RuntimeError as "skip this step"
    (hydrodynamics_behavior.py:191-192)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


def load(path: str | None = None) -> ctypes.CDLL:
    """Load libhydro.so and attach prototypes.  Raises OSError if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("HYDRO_LIBRARY") or LIB_PATH     # HYDRO_LIBRARY: another build of libhydro.so (A/B runs)
    if not os.path.exists(p):
        raise OSError(f"{p} not found: the HIP extension is not built "
                      f"(run `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so, and whichever copy is mapped first serves
    # every later user of that SONAME.  If libhydro.so came first it would bring the system runtime in, torch would
    # then run on a runtime it was not built against, and device calls fail (hipGetDeviceCount -> HYDRO_E_DEVICE).
    # The Python host uses torch for memory and streams anyway, so load it first.
    import torch  # noqa: F401
    lib = ctypes.CDLL(p)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _lib = lib
    return lib


def pointer_table(ptrs) -> ctypes.Array:
    """ctypes array of raw addresses (ints) usable as `const float *const t[N]`."""
    arr = (c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = int(p)
    return arr
