"""Python host of the C ABI: one `HydroEngine` = one `hydro_t` handle on one GPU.

PyTorch is used for plumbing only - device buffers, the current HIP stream and
(in `distributed.py`) the process group.  Every numerical result comes from the
hand-written HIP kernels in `csrc/hydro_kernels.hip` through `libhydro.so`;
there is no CPU or eager-PyTorch fallback.

Layouts: "SoA" tensors are contiguous `(F, N)` float32 device tensors - row f is
field f (orders in include/hydro.h).

Each rule for turning a Python argument into C arguments is written once: `_tiled` (a tiled buffer ->
pointer, tile stride), `_prev_velocity` (None / state buffer / 6-field buffer), `_wrench_tiled_call` and
`_wrench_aos_call` (the direct and the prepared form of a step share one argument list), `_fused_head`
(the fused steps), `_fused_multi_args`, `_rec_tail` and `_applied_control` (the multi-step entries) and `_rows` / `_force_torque` (simulator tensors).  tests/test_engine_calls.py
pins the resulting calls without a GPU.
"""
from __future__ import annotations

import ctypes
import logging

import numpy as np
import torch

from . import _native as nat
from ._native import HydroError

log = logging.getLogger("silver2_isaacsim_amd")
_warp_mode_announced = False
_VEL_BYTES = 7 * nat.TILE * 4          # where the six velocity fields start inside a state tile
_FRAMES = {"world": nat.HYDRO_FRAME_WORLD, "body": nat.HYDRO_FRAME_BODY}      # frame of an applied wrench


def _prebuilt(name: str, args, first: int = 0) -> tuple:
    """`args` (arguments `first`, `first` + 1, ... of C function `name`) as the ctypes values its prototype would
    convert them to on every call: a prepared launch builds them once."""
    return tuple(a if isinstance(a, ctypes.c_void_p) else t(a) for t, a in zip(nat.SIGNATURES[name][1][first:], args))


def _as_soa_tensor(x, fields: int, device: torch.device) -> torch.Tensor:
    """(N,F) or (F,N) array-like -> contiguous (F,N) float32 tensor on `device`."""
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if t.ndim != 2:
        raise ValueError("expected a 2-D array")
    if t.shape[0] != fields and t.shape[1] == fields:
        t = t.t()
    elif t.shape[0] != fields:
        raise ValueError(f"expected {fields} fields, got shape {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


class HydroEngine:
    """Batched replacement for N per-prim calculator objects of the reference
    (`WarpHydrodynamicsWrapper`, warp_hydrodynamics_wrapper.py:5-132)."""

    def __init__(self, capacity: int, device: int | str | torch.device = 0,
                 water_density: float = 1025.0, gravity: float = 9.81):
        self._lib = nat.load()                       # raises if the HIP extension is missing
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise ValueError("HydroEngine runs on a GPU device only (no CPU path)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else 0)
        self.capacity = int(capacity)
        self._h = ctypes.c_void_p()
        rc = self._lib.hydro_create(self.device.index, self.capacity, ctypes.byref(self._h))
        if rc != nat.HYDRO_OK:
            self._h = None
            raise HydroError(rc, f"hydro_create(device={self.device.index}, capacity={capacity}) failed")
        self.n = 0
        self.coeff_dtype = "f32"
        self.semantics = "numba"
        self._tables: dict = {}
        self.sea_waves: int | None = None            # wave components of the sea set with set_sea; None: no sea
        self.spectrum_waves: int | None = None       # wave components of the spectrum set with set_sea_spectrum; None: no spectrum
        self.ensemble_count: int | None = None       # members of the ensemble set with set_sea_ensemble; None: no ensemble
        self.finite_depth: float | None = None       # the depth (m) of the sea set with set_sea_finite_depth; None: no finite-depth sea
        self.current_profile = None                  # the sea.CurrentProfile set with set_current_profile; None: no profile
        self.seabed = None                           # the seabed.Seabed set with set_seabed; None: no bed
        self.set_scene(water_density, gravity)

    # ------------------------------------------------------------------ utils
    def _check(self, rc: int) -> None:
        if rc != nat.HYDRO_OK:
            msg = self._lib.hydro_last_error(self._h)
            raise HydroError(rc, msg.decode() if msg else "")

    def _table(self, t: torch.Tensor, fields: int):
        """Pointer table for a contiguous (fields, N) float32 device tensor (cached)."""
        key = (t.data_ptr(), t.shape[1], fields)
        tab = self._tables.get(key)
        if tab is None:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != fields or t.device != self.device:
                raise ValueError(f"expected contiguous float32 ({fields},N) tensor on {self.device}")
            stride = t.shape[1] * 4
            base = t.data_ptr()
            tab = nat.pointer_table([base + f * stride for f in range(fields)])
            if len(self._tables) > 256:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _stream(self, stream) -> ctypes.c_void_p:
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(int(stream.cuda_stream if hasattr(stream, "cuda_stream") else stream))

    # ------------------------------------------------------------ configuration
    def set_scene(self, water_density: float, gravity: float) -> None:
        self.water_density, self.gravity = float(water_density), float(gravity)
        self._check(self._lib.hydro_set_scene(self._h, self.water_density, self.gravity))

    def set_semantics(self, semantics: str = "numba") -> None:
        """'numba' (default, the parity target) or 'warp': follow the reference's Warp twin where the two
        calculators differ (added-mass rotation, centres of a dry body; include/hydro.h).
        What pins 'warp': the reference's warp_hydrodynamics.py and its wrapper executed under a stand-in for the Warp
        runtime (fp64, zero-initialised locals modelled, quat_rotate = the matrix form; tests/test_warp_semantics.py) -
        not NVIDIA's runtime, its fp32 rounding or its own quat_rotate, against which the wrench moves by up to 1.0e-5 on
        fp32-rounded unit quaternions and at order one on non-unit ones.  Said once per process through the package logger."""
        global _warp_mode_announced
        code = {"numba": nat.HYDRO_SEM_NUMBA, "warp": nat.HYDRO_SEM_WARP}.get(semantics)
        if code is None:
            raise ValueError("semantics must be 'numba' or 'warp'")
        if semantics == "warp" and not _warp_mode_announced:
            _warp_mode_announced = True
            log.warning("semantics='warp': pinned on the reference's warp_hydrodynamics.py executed under an fp64 stand-in for "
                        "the Warp runtime (matrix quat_rotate), not on NVIDIA's runtime; 'numba' is the parity target")
        self._check(self._lib.hydro_set_semantics(self._h, code))
        self.semantics = semantics

    def set_params(self, params, coeff_dtype: str = "f32") -> None:
        """Per-body constants, (N,11) or (11,N): dims(3), cd_lin, cd_ang, damp_lin, damp_ang,
        lift, am_lin, am_ang, mass.  coeff_dtype 'f16' stores the seven coefficients as half."""
        t = _as_soa_tensor(params, nat.PARAM_FIELDS, self.device)
        n = t.shape[1]
        fn = {"f32": self._lib.hydro_set_params_f32, "f16": self._lib.hydro_set_params_f16}[coeff_dtype]
        torch.cuda.current_stream(self.device).synchronize()      # the copy runs on the engine's stream
        self._check(fn(self._h, n, self._table(t, nat.PARAM_FIELDS), 1))
        self.n = n
        self.coeff_dtype = coeff_dtype

    def reserve_soa(self) -> None:
        """Make the engine's plain-SoA copies of the parameters / previous velocity now (82 B per body).  They are
        otherwise made by the first call of an entry that takes plain field pointers (`step_wrench`, `step_components`),
        which then allocates and synchronises once - call this first if that call is to be captured into a HIP graph."""
        self._check(self._lib.hydro_reserve_soa(self._h))

    def set_tuning(self, bodies_per_lane: int = 0, block_threads: int = 0, non_temporal: int = -1,
                   waves_per_simd: int = -1) -> None:
        self._check(self._lib.hydro_set_tuning(self._h, bodies_per_lane, block_threads, non_temporal, waves_per_simd))

    # ------------------------------------------------- previous-velocity state
    def reset_prev_velocity(self) -> None:
        self._check(self._lib.hydro_reset_prev_velocity(self._h))

    def get_prev_velocity(self) -> torch.Tensor:
        """(6, n) copy of the engine-owned previous velocity (checkpoint / resume).  The C call works on the engine's
        private stream: the step that last wrote the records ran on the caller's, so that one is drained first."""
        out = torch.empty((nat.PREV_FIELDS, self.n), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        self._check(self._lib.hydro_get_prev_velocity(self._h, self.n, self._table(out, nat.PREV_FIELDS), 1))
        return out

    def set_prev_velocity(self, prev) -> None:
        t = _as_soa_tensor(prev, nat.PREV_FIELDS, self.device)
        torch.cuda.current_stream(self.device).synchronize()
        self._check(self._lib.hydro_set_prev_velocity(self._h, t.shape[1], self._table(t, nat.PREV_FIELDS), 1))

    # ----------------------------------------------------------------- hot path
    def step_wrench(self, state: torch.Tensor, dt: float, out: torch.Tensor | None = None,
                    prev: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Fused wrench for state (13,N) -> out (6,N) [F|T].  With `prev` (6,N) the caller owns
        the previous velocity (buffer-swap mode, nothing else is written); without it the
        engine's own previous-velocity buffer is read and updated."""
        n = state.shape[1]
        if out is None:
            out = torch.empty((nat.WRENCH_FIELDS, n), dtype=torch.float32, device=self.device)
        st, ot = self._table(state, nat.STATE_FIELDS), self._table(out, nat.WRENCH_FIELDS)
        if prev is None:
            rc = self._lib.hydro_step_wrench(self._h, n, st, float(dt), ot, self._stream(stream))
        else:
            rc = self._lib.hydro_step_wrench_ext(self._h, n, st, self._table(prev, nat.PREV_FIELDS),
                                                 float(dt), ot, self._stream(stream))
        self._check(rc)
        return out

    # ------------------------------------------------- tiled SoA (native layout)
    @staticmethod
    def tiles(n: int) -> int:
        return (int(n) + nat.TILE - 1) // nat.TILE

    def alloc_tiled(self, fields: int, n: int) -> torch.Tensor:
        """Zeroed (tiles, fields, 64) float32 buffer: body i, field f at [i // 64, f, i % 64]."""
        return torch.zeros((self.tiles(n), fields, nat.TILE), dtype=torch.float32, device=self.device)

    def _tiled(self, t: torch.Tensor, fields: int, n: int):
        """Validate a (>= tiles(n), fields, 64) buffer - the last test reads "fewer than tiles(n) tiles" - and return its
        (address, tile stride in floats)."""
        if (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.ndim != 3
                or t.shape[1] != fields or t.shape[2] != nat.TILE or t.shape[0] * nat.TILE < n):
            raise ValueError(f"expected contiguous float32 (>= {self.tiles(n)}, {fields}, {nat.TILE}) tensor on {self.device}")
        return t.data_ptr(), fields * nat.TILE

    def _prev_velocity(self, prev: torch.Tensor | None, n: int):
        """(address, tile stride) of a step's previous velocity: None = engine-owned; a 13-field STATE buffer = its six
        velocity fields, in place; anything else is held to be a 6-field buffer."""
        if prev is None:
            return None, 0
        if prev.shape[1] == nat.STATE_FIELDS:
            ptr, stride = self._tiled(prev, nat.STATE_FIELDS, n)
            return ptr + _VEL_BYTES, stride
        return self._tiled(prev, nat.PREV_FIELDS, n)

    def to_tiled(self, soa: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """(F,N) plain SoA -> (tiles,F,64) tiled, on device (hydro_repack)."""
        f, n = soa.shape
        if out is None:
            out = self.alloc_tiled(f, n)
        ptr, stride = self._tiled(out, f, n)
        self._check(self._lib.hydro_repack(self._h, n, f, self._table(soa, f), ptr, stride, 1, self._stream(stream)))
        return out

    def from_tiled(self, tiled: torch.Tensor, n: int, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        f = tiled.shape[1]
        ptr, stride = self._tiled(tiled, f, n)
        if out is None:
            out = torch.empty((f, n), dtype=torch.float32, device=self.device)
        self._check(self._lib.hydro_repack(self._h, n, f, self._table(out, f), ptr, stride, 0, self._stream(stream)))
        return out

    def _check_ke_out(self, ke_out: torch.Tensor) -> None:
        if ke_out.dtype != torch.float64 or ke_out.device != self.device or ke_out.numel() < 2 or not ke_out.is_contiguous():
            raise ValueError(f"ke_out: expected a contiguous float64 tensor of 2 elements on {self.device}")

    def _wrench_tiled_call(self, state, n, dt, out, prev, stream, ke_out, rotational, time=None, irr=False):
        """(name, args, out) of one `hydro_step_wrench_tiled[_ke | _sea | _irr]` launch: the buffers validated, `out` allocated
        when None, the stream resolved now.  `time` (seconds) selects the `_sea` entry - with `irr` its `_irr` sibling - which
        takes it in front of the stream."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.WRENCH_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
        p_ptr, p_stride = self._prev_velocity(prev, n)
        args = (self._h, n, s_ptr, s_stride, p_ptr, p_stride, float(dt), o_ptr, o_stride)
        if time is not None:
            if ke_out is not None:
                raise ValueError("the sea entry does not sample the kinetic energy (ke_out must be None)")
            return "hydro_step_wrench_tiled_irr" if irr else "hydro_step_wrench_tiled_sea", args + (float(time), self._stream(stream)), out
        if ke_out is None:
            return "hydro_step_wrench_tiled", args + (self._stream(stream),), out
        self._check_ke_out(ke_out)                      # the variant that samples the kinetic energy of `state` on the way
        return "hydro_step_wrench_tiled_ke", args + (int(bool(rotational)), ke_out.data_ptr(), self._stream(stream)), out

    def step_wrench_tiled(self, state: torch.Tensor, n: int, dt: float, out: torch.Tensor | None = None,
                          prev: torch.Tensor | None = None, stream=None, ke_out: torch.Tensor | None = None,
                          rotational: bool = True) -> torch.Tensor:
        """Fused wrench on tiled buffers: state (tiles,13,64) -> out (tiles,6,64).
        prev: None = engine-owned previous velocity (read + updated); a (tiles,6,64) tensor; or a
        (tiles,13,64) STATE tensor whose velocity fields are used in place (ping-pong integrator:
        pass the previous step's state buffer - nothing is copied).
        ke_out (float64, 2 elements, on the device): the kernel also samples the kinetic energy of `state` - the
        bodies it holds in registers anyway, no second pass - into ke_out[0:2] = [translational, rotational]."""
        name, args, out = self._wrench_tiled_call(state, n, dt, out, prev, stream, ke_out, rotational)
        self._check(getattr(self._lib, name)(*args))
        return out

    def step_wrench_tiled_sea(self, state: torch.Tensor, n: int, dt: float, time: float, out: torch.Tensor | None = None,
                              prev: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """`step_wrench_tiled` through the sea set with `set_sea`, at `time` seconds (hydro_step_wrench_tiled_sea): the wrench
        of the state relative to the local water - depth below the local surface, velocity against current and orbital
        velocity.  The engine-owned previous velocity (prev=None) receives the TRUE velocity; a caller-owned `prev` is only
        read.  Without a sea the call is step_wrench_tiled."""
        name, args, out = self._wrench_tiled_call(state, n, dt, out, prev, stream, None, True, time)
        self._check(getattr(self._lib, name)(*args))
        return out

    def step_wrench_tiled_irr(self, state: torch.Tensor, n: int, dt: float, time: float, out: torch.Tensor | None = None,
                              prev: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """`step_wrench_tiled_sea` through whichever sea the engine holds, at `time` seconds (hydro_step_wrench_tiled_irr): the
        finite-depth sea of `set_sea_finite_depth`, the ensemble of `set_sea_ensemble` (block m of the bodies against member m),
        the spectrum of `set_sea_spectrum`, or the sea of `set_sea`.  The engine-owned previous velocity (prev=None) receives
        the TRUE velocity; a caller-owned `prev` is only read.  Without any sea the call is step_wrench_tiled."""
        name, args, out = self._wrench_tiled_call(state, n, dt, out, prev, stream, None, True, time, irr=True)
        self._check(getattr(self._lib, name)(*args))
        return out

    def holds_irregular_sea(self) -> bool:
        """Whether the last seas set successfully through this object leave a spectrum, an ensemble or a finite-depth sea in
        the engine: the prepared steps then issue the `_irr` entries for a `time`, the `_sea` entries otherwise."""
        return self.spectrum_waves is not None or self.ensemble_count is not None or self.finite_depth is not None

    def prepare_step_wrench_tiled(self, state: torch.Tensor, n: int, dt: float, out: torch.Tensor | None = None,
                                  prev: torch.Tensor | None = None, stream=None, ke_out: torch.Tensor | None = None,
                                  rotational: bool = True):
        """Build the launch of `step_wrench_tiled` ONCE (same validation, same arguments: `_wrench_tiled_call`) and
        return a callable `step(time=None)` that issues it again (same buffers, same stream - the one current now if
        `stream` is None).  For step loops over small scenes, where the per-call Python work (shape checks, ctypes
        conversions: ~10 us) exceeds the kernel (~3 us at 4 096 bodies): the prepared call costs ~4 us of host time.
        `step()` is that launch, argument for argument; `step(time)` is `step_wrench_tiled_sea` at `time` seconds on the
        same buffers (not with ke_out) - `step_wrench_tiled_irr` while the engine holds a spectrum, an ensemble or a
        finite-depth sea (`holds_irregular_sea`, asked at every step).  The callable returns `out`; errors raise HydroError as usual."""
        name, args, out = self._wrench_tiled_call(state, n, dt, out, prev, stream, ke_out, rotational)
        fn, args = getattr(self._lib, name), _prebuilt(name, args)
        keep = (state, prev, out, ke_out)               # the buffers must outlive the callable
        check = self._check
        sea_fn, irr_fn, sea_args = None, None, None
        if ke_out is None:                              # the same argument list with the time in front of the stream
            sea_fn, irr_fn, sea_args = self._lib.hydro_step_wrench_tiled_sea, self._lib.hydro_step_wrench_tiled_irr, (args[:-1], args[-1])
        irregular = self.holds_irregular_sea

        def step(time=None):
            if self._h is None:                         # engine closed: the captured handle is gone
                raise HydroError(nat.HYDRO_E_STATE, "engine is closed")
            if time is None:
                rc = fn(*args)
            elif sea_fn is None:
                raise ValueError("the sea entry does not sample the kinetic energy (prepared with ke_out)")
            else:
                rc = (irr_fn if irregular() else sea_fn)(*sea_args[0], ctypes.c_double(time), sea_args[1])
            if rc:
                check(rc)
            return keep[2]
        return step

    @staticmethod
    def prepare_step_wrench_tiled_batch(engines, states, dt: float, outs=None, prevs=None, ns=None, stream=None):
        """k independent scenes in ONE launch (hydro_step_wrench_tiled_batch): engines[i] steps states[i] (tiled
        (tiles,13,64)) into outs[i] ((tiles,6,64), allocated when None) with prevs[i] as the previous velocity (tiled
        6-field buffers or the velocity fields of a previous state buffer; None = every engine's own).  Same bits as k
        single calls; one ramp and drain for all of them.  Returns (step, outs): `step()` re-issues the launch on the
        stream current at the time of the call (arguments are validated here, once)."""
        k = len(engines)
        if not 1 <= k <= nat.BATCH_MAX or len(states) != k:
            raise ValueError(f"1 .. {nat.BATCH_MAX} scenes per launch, one state buffer each")
        ns = list(ns) if ns is not None else [e.n for e in engines]
        outs = list(outs) if outs is not None else [e.alloc_tiled(nat.WRENCH_FIELDS, n) for e, n in zip(engines, ns)]
        arr = (nat.Scene * k)()
        keep = []
        for i, (e, st, n, out) in enumerate(zip(engines, states, ns, outs)):
            sc = arr[i]
            sc.engine, sc.n = e._h, n
            sc.state, sc.state_tile_stride = e._tiled(st, nat.STATE_FIELDS, n)
            sc.wrench, sc.wrench_tile_stride = e._tiled(out, nat.WRENCH_FIELDS, n)
            if prevs is not None:                                   # else NULL, 0: every engine's own
                sc.prev, sc.prev_tile_stride = e._prev_velocity(prevs[i], n)
                keep.append(prevs[i])
            keep += [st, out]
        first = engines[0]
        fn, dtc = first._lib.hydro_step_wrench_tiled_batch, ctypes.c_double(dt)

        def step(stream=stream):
            rc = fn(k, arr, dtc, first._stream(stream))
            if rc:
                first._check(rc)
            return outs
        step._keep = (keep, arr)
        return step, outs

    @staticmethod
    def step_wrench_tiled_batch(engines, states, dt: float, outs=None, prevs=None, ns=None, stream=None):
        """One launch for k scenes; returns the list of wrench buffers.  See prepare_step_wrench_tiled_batch."""
        step, outs = HydroEngine.prepare_step_wrench_tiled_batch(engines, states, dt, outs, prevs, ns, stream)
        step()
        return outs

    def _fused_head(self, state, prev_state, n, dt, state_out):
        """What the three fused steps share: the state buffers validated, `state_out` defaulted to `prev_state`.
        Returns (state_out, the tile stride of a state buffer, the leading C arguments up to `dt`)."""
        s_ptr, st = self._tiled(state, nat.STATE_FIELDS, n)
        p_ptr, _ = self._tiled(prev_state, nat.STATE_FIELDS, n)
        if state_out is None:
            state_out = prev_state
        self._tiled(state_out, nat.STATE_FIELDS, n)
        return state_out, st, (self._h, n, s_ptr, st, p_ptr + _VEL_BYTES, st, float(dt))

    def step_fused_tiled(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float,
                         state_out: torch.Tensor | None = None, wrench: torch.Tensor | None = None,
                         implicit_drag: bool = False, stream=None, ke_out: torch.Tensor | None = None,
                         rotational: bool = True):
        """Wrench + integrator in one kernel.  `prev_state` (tiles,13,64) supplies the previous velocity;
        `state_out` defaults to `prev_state` itself (ping-pong: the old buffer receives the new state).
        ke_out (float64, 2 elements, device): also sample the kinetic energy of the NEW state into it."""
        state_out, st, head = self._fused_head(state, prev_state, n, dt, state_out)
        w_ptr, w_stride = self._tiled(wrench, nat.WRENCH_FIELDS, n) if wrench is not None else (None, 0)
        tail = (state_out.data_ptr(), st, w_ptr, w_stride, int(bool(implicit_drag)))
        if ke_out is None:
            self._check(self._lib.hydro_step_fused_tiled(*head, *tail, self._stream(stream)))
        else:
            self._check_ke_out(ke_out)
            self._check(self._lib.hydro_step_fused_tiled_ke(*head, *tail, int(bool(rotational)), ke_out.data_ptr(),
                                                            self._stream(stream)))
        return state_out

    def _fused_multi_args(self, state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational):
        """(state_out, the arguments `hydro_step_fused_tiled_multi[_rec]` share): the final state goes to `state_out`,
        the velocity of the step before the last one into the velocity fields of `state`."""
        state_out, st, head = self._fused_head(state, prev_state, n, dt, state_out)
        if ke_out is not None:
            self._check_ke_out(ke_out)
        return state_out, head + (int(steps), state_out.data_ptr(), st, state.data_ptr() + _VEL_BYTES, st,
                                  int(bool(implicit_drag)), int(bool(rotational)),
                                  ke_out.data_ptr() if ke_out is not None else None)

    def _rec_tail(self, log, every, phase, row0):
        """The recorder's arguments of `hydro_step_fused_tiled_multi_rec` / `_app` (log .. rows_written_host) and the
        counter the call fills in.  `log` None (the applied entry only): no recording."""
        written = ctypes.c_int64(0)
        if log is None:
            return (None, 0, 0, nat.STATE_FIELDS, 1, 1, 0, ctypes.byref(written)), written
        if (log.dim() != 3 or log.dtype != torch.float32 or not log.is_contiguous() or log.device != self.device
                or log.shape[1] not in (nat.STATE_FIELDS, nat.STATE_FIELDS + nat.WRENCH_FIELDS)):
            raise ValueError("log must be a contiguous float32 (rows, 13 | 19, columns) tensor on the engine's device")
        return (log.data_ptr(), log.shape[2], log.shape[0], log.shape[1], int(every), int(phase), int(row0),
                ctypes.byref(written)), written

    def _recorded_multi(self, entry, multi, rec, stream, extra=lambda: ()) -> int:
        """One call of a multi-step entry that can record: `multi` are `_fused_multi_args`' arguments, `rec` `_rec_tail`'s,
        `extra()` gives what the entry takes between `rows_written_host` and `stream` (built, and so validated, after the
        other two).  Returns the number of rows written."""
        _, args = self._fused_multi_args(*multi)
        tail, written = self._rec_tail(*rec)
        self._check(entry(*args, *tail, *extra(), self._stream(stream)))
        return written.value

    def step_fused_tiled_multi(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int,
                               state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                               ke_out: torch.Tensor | None = None, rotational: bool = True):
        """`steps` closed-loop steps in one kernel, every body carried through them in registers (same bits as `steps`
        calls of step_fused_tiled).  Buffers as step_fused_tiled: `prev_state` supplies the previous velocity and, by
        default, receives the final state; the velocity fields of `state` receive the velocity of the step before the
        last one, so that after the call (state_out, state) are the (current, previous) pair of the next call.
        ke_out: also sample the kinetic energy of the final state."""
        state_out, args = self._fused_multi_args(state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational)
        self._check(self._lib.hydro_step_fused_tiled_multi(*args, self._stream(stream)))
        return state_out

    def set_watch(self, bodies) -> int:
        """The trajectory recorder's watch list (hydro_set_watch): strictly ascending body indices below the capacity, at most
        `_native.WATCH_MAX` of them; body bodies[j] records into column j of the log.  None or an empty list clears it.
        Synchronous.  Returns the number of watched bodies."""
        if bodies is None or len(bodies) == 0:
            self._check(self._lib.hydro_set_watch(self._h, 0, None))
            return 0
        arr = (ctypes.c_int64 * len(bodies))(*[int(b) for b in bodies])
        self._check(self._lib.hydro_set_watch(self._h, len(bodies), arr))
        return int(self._lib.hydro_watch_count(self._h))

    @property
    def watch_count(self) -> int:
        return int(self._lib.hydro_watch_count(self._h))

    def step_fused_tiled_multi_rec(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int,
                                   log: torch.Tensor, every: int, phase: int, row0: int,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi that also records the watched bodies (set_watch) from inside the kernel: after local step
        k = phase, phase + every, ... of this launch, into rows row0, row0 + 1, ... of `log`, a contiguous float32 device
        tensor (rows, 13 | 19, columns >= watch count) - 19 fields: the state, then the wrench that produced it.  State,
        previous-velocity and kinetic-energy bits are those of step_fused_tiled_multi.  Returns the number of rows written."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_rec,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream)

    def step_fused_tiled_multi_applied(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int,
                                       applied: torch.Tensor | None, frame: str = "body", log: torch.Tensor | None = None,
                                       every: int = 1, phase: int = 1, row0: int = 0,
                                       state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                       ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi with an external force and torque on every body (hydro_step_fused_tiled_multi_app):
        `applied` is a tiled (tiles, 6, 64) buffer of [Fx Fy Fz | Tx Ty Tz] per body - force at, torque about the body
        origin - added to the hydrodynamic wrench inside every one of the `steps` steps, held constant in its frame:
        frame="world" as it stands, frame="body" turned by the body's attitude at each step (a thruster).  steps=1 is the
        single-step form.  applied=None is the unapplied step.  `log` (with every / phase / row0, see
        step_fused_tiled_multi_rec) also records the watched bodies; the wrench it logs is the total.  Returns the number
        of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_app,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._applied_control(applied, frame, None, n)[:3])

    def step_fused_tiled_multi_controlled(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int,
                                          control: torch.Tensor | None, applied: torch.Tensor | None = None, frame: str = "body",
                                          log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                          state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                          ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_applied with a pose-hold feedback law on every body (hydro_step_fused_tiled_multi_ctl):
        `control` is a tiled (tiles, 17, 64) buffer of [p*(3) | q*(4, xyzw) | kp_lin(3) | kd_lin(3) | kp_ang | kd_ang |
        f_max | t_max] per body.  In every one of the `steps` steps the kernel forms, from the state that step starts from,
        a clamped PD force towards p* and torque towards q* (the law and its order: include/hydro.h) and adds them to the
        hydrodynamic wrench, after `applied` if there is one.  control=None is step_fused_tiled_multi_applied.  Returns the
        number of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_ctl,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._applied_control(applied, frame, control, n))

    def _applied_control(self, applied, frame, control, n):
        """The arguments `applied .. control_tile_stride` of `hydro_step_fused_tiled_multi_ctl` / `_sea` / `_bed` (the first three:
        `_app`'s): either buffer may be None (NULL, stride 0)."""
        code = _FRAMES.get(frame)
        if code is None:
            raise ValueError("frame must be 'world' or 'body'")
        a_ptr, a_stride = self._tiled(applied, nat.WRENCH_FIELDS, n) if applied is not None else (None, 0)
        c_ptr, c_stride = self._tiled(control, nat.CTL_FIELDS, n) if control is not None else (None, 0)
        return a_ptr, a_stride, code, c_ptr, c_stride

    # ------------------------------------------------------------------ sea state
    def set_sea(self, sea) -> None:
        """The scene's moving water (hydro_set_sea; the model: include/hydro.h): `sea` has `current` (3 floats, m/s, world
        frame) and `waves`, up to `_native.SEA_WAVES_MAX` rows (amplitude, kx, ky, omega, phase) - a `sea.SeaState`.  None clears
        it.  The `step_fused_tiled_multi_sea` family, `step_wrench_tiled_sea`, `step_wrench_aos_sea` and `sea_sample[_at]` see the
        sea; every other entry steps through still water.  Synchronous: the copy runs on the engine's
        stream, so launches of this engine still in flight elsewhere are the caller's to wait for."""
        if sea is None:
            self._check(self._lib.hydro_set_sea(self._h, None))
            self.sea_waves = None
            return
        waves = [tuple(float(x) for x in w) for w in sea.waves]
        if len(waves) > nat.SEA_WAVES_MAX or any(len(w) != 5 for w in waves):
            raise ValueError(f"a sea has at most {nat.SEA_WAVES_MAX} wave components of (amplitude, kx, ky, omega, phase)")
        c = nat.Sea()
        c.current[:] = [float(x) for x in sea.current]
        c.waves = len(waves)
        for j, w in enumerate(waves):
            c.wave[j] = nat.SeaWave(*w)
        self._check(self._lib.hydro_set_sea(self._h, ctypes.byref(c)))
        self.sea_waves = len(waves)

    def sea_sample(self, state: torch.Tensor, n: int, step_index: int, dt: float, out: torch.Tensor | None = None,
                   stream=None) -> torch.Tensor:
        """The water each body of the tiled `state` meets at the start of step `step_index` (hydro_sea_sample): a tiled
        (tiles, 4, 64) buffer of [eta, u_x, u_y, u_z] - surface elevation above the body and water velocity at its centre,
        exactly the values `step_fused_tiled_multi_sea` uses for that step."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.SEA_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.SEA_FIELDS, n)
        self._check(self._lib.hydro_sea_sample(self._h, n, s_ptr, s_stride, int(step_index), float(dt), o_ptr, o_stride,
                                               self._stream(stream)))
        return out

    def sea_sample_at(self, state: torch.Tensor, n: int, time: float, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The water each body of the tiled `state` meets at `time` seconds: exactly the [eta, u_x, u_y, u_z] that
        `step_wrench_tiled_sea` / `step_wrench_aos_sea` use at that time.  `sea_sample` with (step_index, dt) = (1, time) -
        (double)1 * time == time exactly - or (0, 1.0) at time 0 (include/hydro.h, "Sea state, open loop")."""
        time = float(time)
        return self.sea_sample(state, n, *((1, time) if time > 0.0 else (0, 1.0)), out=out, stream=stream)

    def irregular_sea_sample_at(self, state: torch.Tensor, n: int, time: float, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The water each body of the tiled `state` meets at `time` seconds in the spectrum, the ensemble or the finite-depth sea
        the engine holds: exactly the [eta, u_x, u_y, u_z] that `step_wrench_tiled_irr` / `step_wrench_aos_irr` use at that time.
        The matching `sea_finite_depth_sample`, `sea_ensemble_sample` or `sea_spectrum_sample` with (step_index, dt) = (1, time) -
        (double)1 * time == time exactly - or (0, 1.0) at time 0 (include/hydro.h, "Irregular sea in the open-loop steps")."""
        time = float(time)
        sample = (self.sea_finite_depth_sample if self.finite_depth is not None
                  else self.sea_ensemble_sample if self.ensemble_count is not None else self.sea_spectrum_sample)
        return sample(state, n, *((1, time) if time > 0.0 else (0, 1.0)), out=out, stream=stream)

    def step_fused_tiled_multi_sea(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_controlled through the sea set with `set_sea` (hydro_step_fused_tiled_multi_sea): in every
        step the hydrodynamic wrench is that of the state RELATIVE to the local water - depth below the local surface,
        velocity against current and wave orbital velocity - while integrator, applied wrench, pose hold and recorder act
        on the true state.  `step0`: the index of this launch's first step (the wave phase is (step0 + k) * dt inside the
        launch).  control, applied and log are each optional; without a sea the call is step_fused_tiled_multi_controlled.
        Returns the number of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_sea,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: (*self._applied_control(applied, frame, control, n), int(step0)))

    # ------------------------------------------------------------------ sea spectrum
    def set_sea_spectrum(self, spectrum) -> None:
        """The scene's irregular sea (hydro_set_sea_spectrum; include/hydro.h, "Sea spectrum"): `spectrum` has `current` and
        `waves`, up to `_native.SPECTRUM_WAVES_MAX` rows (amplitude, kx, ky, omega, phase) - a `sea.SeaSpectrum`.  None clears it.
        `step_fused_tiled_multi_irr` (and the rungs above it), `sea_spectrum_sample`, `step_wrench_tiled_irr` and
        `step_wrench_aos_irr` see the spectrum.  A spectrum and the sea of `set_sea`
        exclude each other: the library refuses one while the other is set.  Synchronous, like `set_sea`."""
        if spectrum is None:
            self._check(self._lib.hydro_set_sea_spectrum(self._h, None))
            self.spectrum_waves = None
            return
        waves = [tuple(float(x) for x in w) for w in spectrum.waves]
        if len(waves) > nat.SPECTRUM_WAVES_MAX or any(len(w) != 5 for w in waves):
            raise ValueError(f"a sea spectrum has at most {nat.SPECTRUM_WAVES_MAX} wave components of (amplitude, kx, ky, omega, phase)")
        rows = (nat.SeaWave * len(waves))(*[nat.SeaWave(*w) for w in waves])     # (alive until the call returns: the library copies)
        c = nat.SeaSpectrum()
        c.current[:] = [float(x) for x in spectrum.current]
        c.waves = len(waves)
        c.wave = ctypes.cast(rows, ctypes.POINTER(nat.SeaWave)) if waves else None
        self._check(self._lib.hydro_set_sea_spectrum(self._h, ctypes.byref(c)))
        self.spectrum_waves = len(waves)

    def sea_spectrum_sample(self, state: torch.Tensor, n: int, step_index: int, dt: float, out: torch.Tensor | None = None,
                            stream=None) -> torch.Tensor:
        """`sea_sample` against the spectrum set with `set_sea_spectrum` (hydro_sea_spectrum_sample): exactly the
        [eta, u_x, u_y, u_z] `step_fused_tiled_multi_irr` uses for step `step_index`."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.SEA_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.SEA_FIELDS, n)
        self._check(self._lib.hydro_sea_spectrum_sample(self._h, n, s_ptr, s_stride, int(step_index), float(dt), o_ptr, o_stride,
                                                        self._stream(stream)))
        return out

    def step_fused_tiled_multi_irr(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   mooring: torch.Tensor | None = None, mooring_layers: int = 1,
                                   tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                   extremes: torch.Tensor | None = None,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_spread through the irregular sea set with `set_sea_spectrum`
        (hydro_step_fused_tiled_multi_irr): the arguments and the rules are step_fused_tiled_multi_spread's, every option
        optional, and the hydrodynamic wrench of every step is that of the state relative to the spectrum's water at
        (step0 + k) * dt.  Without a spectrum the call is step_fused_tiled_multi_spread.  Returns the number of rows written
        (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_irr,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._spread_tail(n, step0, mooring, mooring_layers, tether, layers, peaks, extremes, control, applied, frame))

    # ------------------------------------------------------------------ statistics
    def alloc_statistics(self, n: int) -> torch.Tensor:
        """Zeroed statistics record for n bodies - the reset record: (tiles, 11, 64) float32 = 2 816 B per tile, holding per tile
        `{ double sums[4][64]; uint32_t words[3][64]; }` (include/hydro.h, "Statistics"; `statistics.unpack` reads it)."""
        return self.alloc_tiled(nat.STAT_FIELDS, n)

    def statistics_reset(self, statistics: torch.Tensor, n: int, stream=None) -> torch.Tensor:
        """Empty the statistics record of bodies 0 .. n - 1: sums +0.0, words 0 (hydro_statistics_reset).  Asynchronous."""
        p, stride = self._tiled(statistics, nat.STAT_FIELDS, n)
        self._check(self._lib.hydro_statistics_reset(self._h, n, p, stride, self._stream(stream)))
        return statistics

    def step_fused_tiled_multi_stat(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                    statistics: torch.Tensor | None = None, levels: torch.Tensor | None = None,
                                    channel_a: int = nat.STAT_Z, channel_b: int = nat.STAT_TENSION,
                                    mooring: torch.Tensor | None = None, mooring_layers: int = 1,
                                    tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                    extremes: torch.Tensor | None = None,
                                    control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                    log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                    state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                    ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_irr that also keeps each body's running response statistics
        (hydro_step_fused_tiled_multi_stat): `statistics` is the record of `alloc_statistics` / `statistics_reset`, read at
        the start of the launch and written at its end, so it accumulates over launches; `levels` the tiled (tiles, 2, 64)
        reference levels of the two channel slots; `channel_a` / `channel_b` one of `_native.STAT_X .. STAT_TENSION`.  After
        every step the sample of each channel enters its sums and its up-crossing count (include/hydro.h, "Statistics").
        Nothing feeds back: everything else the launch writes is step_fused_tiled_multi_irr's bits, and statistics=None IS that
        call.  Returns the number of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_stat,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._stat_tail(n, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                                            peaks, extremes, control, applied, frame))

    def _stat_tail(self, n, step0, statistics, levels, channel_a, channel_b, *spread):
        """The arguments `applied .. step0` of `hydro_step_fused_tiled_multi_stat` / `_ens`: `_spread_tail`'s with the statistics
        group in front of step0."""
        tail = self._spread_tail(n, step0, *spread)
        s_ptr, s_stride = self._tiled(statistics, nat.STAT_FIELDS, n) if statistics is not None else (None, 0)
        l_ptr, l_stride = self._tiled(levels, nat.STAT_LEVEL_FIELDS, n) if levels is not None else (None, 0)
        return (*tail[:-1], s_ptr, s_stride, l_ptr, l_stride, int(channel_a), int(channel_b), tail[-1])

    # ------------------------------------------------------------------ sea ensemble
    def set_sea_ensemble(self, ensemble) -> None:
        """The scene's sea ensemble (hydro_set_sea_ensemble; include/hydro.h, "Sea ensemble"): `ensemble` has `members`, up to
        `_native.SEA_ENSEMBLE_MAX` spectra of equally many components (each with `current` and `waves`, as `set_sea_spectrum` takes
        them), and `bodies_per_sea`, a multiple of 64 - a `sea.SeaEnsemble`.  Bodies m * bodies_per_sea .. step through member m.
        None clears it.  `step_fused_tiled_multi_ens`, `sea_ensemble_sample`, `step_wrench_tiled_irr` and `step_wrench_aos_irr` see
        the ensemble; an ensemble, a spectrum and
        the sea of `set_sea` exclude each other.  Synchronous, like `set_sea`."""
        if ensemble is None:
            self._check(self._lib.hydro_set_sea_ensemble(self._h, None, 0, 0))
            self.ensemble_count = None
            return
        c, rows = self._c_members(ensemble.members)                                # (alive until the call returns: the library copies)
        self._check(self._lib.hydro_set_sea_ensemble(self._h, c, len(rows), int(ensemble.bodies_per_sea)))
        self.ensemble_count = len(rows)

    @staticmethod
    def _c_members(members):
        """(the array of hydro_sea_spectrum_t that `hydro_set_sea_ensemble` / `_finite_depth` take, the rows that keep it alive)."""
        members = list(members)
        rows = []
        c = (nat.SeaSpectrum * max(len(members), 1))()
        for m, member in enumerate(members):
            waves = [tuple(float(x) for x in w) for w in member.waves]
            if len(waves) > nat.SPECTRUM_WAVES_MAX or any(len(w) != 5 for w in waves):
                raise ValueError(f"a sea spectrum has at most {nat.SPECTRUM_WAVES_MAX} wave components of (amplitude, kx, ky, omega, phase)")
            rows.append((nat.SeaWave * max(len(waves), 1))(*[nat.SeaWave(*w) for w in waves]))
            c[m].current[:] = [float(x) for x in member.current]
            c[m].waves = len(waves)
            c[m].wave = ctypes.cast(rows[-1], ctypes.POINTER(nat.SeaWave)) if waves else None
        return c, rows

    def sea_ensemble_sample(self, state: torch.Tensor, n: int, step_index: int, dt: float, out: torch.Tensor | None = None,
                            stream=None) -> torch.Tensor:
        """`sea_spectrum_sample` with each body read against its member of the ensemble set with `set_sea_ensemble`
        (hydro_sea_ensemble_sample): exactly the [eta, u_x, u_y, u_z] `step_fused_tiled_multi_ens` uses for step `step_index`."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.SEA_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.SEA_FIELDS, n)
        self._check(self._lib.hydro_sea_ensemble_sample(self._h, n, s_ptr, s_stride, int(step_index), float(dt), o_ptr, o_stride,
                                                        self._stream(stream)))
        return out

    def step_fused_tiled_multi_ens(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   statistics: torch.Tensor | None = None, levels: torch.Tensor | None = None,
                                   channel_a: int = nat.STAT_Z, channel_b: int = nat.STAT_TENSION,
                                   mooring: torch.Tensor | None = None, mooring_layers: int = 1,
                                   tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                   extremes: torch.Tensor | None = None,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_stat through the sea ensemble set with `set_sea_ensemble` (hydro_step_fused_tiled_multi_ens):
        the arguments and the rules are step_fused_tiled_multi_stat's, every option optional, and each block of
        `bodies_per_sea` bodies steps through its own member - bit for bit the step it takes in step_fused_tiled_multi_stat
        under `set_sea_spectrum(member)`.  Without an ensemble the call IS step_fused_tiled_multi_stat.  Returns the number of
        rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_ens,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._stat_tail(n, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                                            peaks, extremes, control, applied, frame))

    # ------------------------------------------------------------------ finite-depth sea
    def set_sea_finite_depth(self, sea, n: int | None = None) -> None:
        """The scene's finite-depth sea (hydro_set_sea_finite_depth; include/hydro.h, "Finite-depth sea"): `sea` is a
        `sea.SeaEnsemble` with a `depth` - its members, its `bodies_per_sea` - or a `sea.SeaSpectrum` with a `depth`, which rides as
        ONE member whose block covers `n` bodies (default: the engine's capacity).  The orbital velocity follows cosh / sinh of
        the height above the bed; the surface is the deep model's.  None clears it.  `step_fused_tiled_multi_fd`,
        `sea_finite_depth_sample`, `step_wrench_tiled_irr` and `step_wrench_aos_irr` see it; it, an ensemble, a spectrum and the sea
        of `set_sea` exclude each other.  Synchronous, like `set_sea`."""
        if sea is None:
            self._check(self._lib.hydro_set_sea_finite_depth(self._h, None, 0, 0, 0.0))
            self.finite_depth = None
            return
        if getattr(sea, "depth", None) is None:
            raise ValueError("a finite-depth sea needs a depth (SeaSpectrum(depth=), jonswap(..., depth=))")
        if hasattr(sea, "members"):
            members, per_sea = sea.members, int(sea.bodies_per_sea)
        else:
            members, per_sea = [sea], 64 * max(1, -(-(self.capacity if n is None else int(n)) // 64))
        c, rows = self._c_members(members)                                         # (alive until the call returns: the library copies)
        self._check(self._lib.hydro_set_sea_finite_depth(self._h, c, len(rows), per_sea, float(sea.depth)))
        self.finite_depth = float(sea.depth)

    def sea_finite_depth_sample(self, state: torch.Tensor, n: int, step_index: int, dt: float, out: torch.Tensor | None = None,
                                stream=None) -> torch.Tensor:
        """`sea_ensemble_sample` against the finite-depth sea set with `set_sea_finite_depth` (hydro_sea_finite_depth_sample):
        exactly the [eta, u_x, u_y, u_z] `step_fused_tiled_multi_fd` uses for step `step_index`."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.SEA_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.SEA_FIELDS, n)
        self._check(self._lib.hydro_sea_finite_depth_sample(self._h, n, s_ptr, s_stride, int(step_index), float(dt), o_ptr, o_stride,
                                                            self._stream(stream)))
        return out

    def step_fused_tiled_multi_fd(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                  statistics: torch.Tensor | None = None, levels: torch.Tensor | None = None,
                                  channel_a: int = nat.STAT_Z, channel_b: int = nat.STAT_TENSION,
                                  mooring: torch.Tensor | None = None, mooring_layers: int = 1,
                                  tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                  extremes: torch.Tensor | None = None,
                                  control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                  log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                  state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                  ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_ens through the finite-depth sea set with `set_sea_finite_depth`
        (hydro_step_fused_tiled_multi_fd): the arguments and the rules are step_fused_tiled_multi_ens's, every option optional.
        Without a finite-depth sea the call IS step_fused_tiled_multi_ens.  Returns the number of rows written (0 without a
        log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_fd,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._stat_tail(n, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                                            peaks, extremes, control, applied, frame))

    # ------------------------------------------------------------------ current profile
    def set_current_profile(self, profile) -> None:
        """The scene's sheared current (hydro_set_current_profile; include/hydro.h, "Current profile"): `profile` is a
        `sea.CurrentProfile` - up to 16 knots (z_l, V_l), piecewise linear, constant beyond the ends - added to the water of the
        finite-depth sea for every member.  None (or a profile without knots) clears it.  Only `step_fused_tiled_multi_shear` and
        `current_profile_sample` see it, and only while a finite-depth sea is set.  Synchronous, like `set_sea`."""
        if profile is None or len(profile.z) == 0:
            self._check(self._lib.hydro_set_current_profile(self._h, None))
            self.current_profile = None
            return
        knots = len(profile.z)
        z = (ctypes.c_float * knots)(*[float(x) for x in profile.z])               # (alive until the call returns: the library copies)
        v = (ctypes.c_float * (3 * knots))(*[float(x) for row in profile.v for x in row])
        c = nat.CurrentProfile(knots, ctypes.cast(z, ctypes.POINTER(ctypes.c_float)), ctypes.cast(v, ctypes.POINTER(ctypes.c_float)))
        self._check(self._lib.hydro_set_current_profile(self._h, ctypes.byref(c)))
        self.current_profile = profile

    def current_profile_sample(self, state: torch.Tensor, n: int, step_index: int, dt: float, out: torch.Tensor | None = None,
                               stream=None) -> torch.Tensor:
        """`sea_finite_depth_sample` with the current profile in u (hydro_current_profile_sample): exactly the
        [eta, u_x, u_y, u_z] `step_fused_tiled_multi_shear` uses for step `step_index`.  Without a profile, the bits of
        `sea_finite_depth_sample`."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.SEA_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.SEA_FIELDS, n)
        self._check(self._lib.hydro_current_profile_sample(self._h, n, s_ptr, s_stride, int(step_index), float(dt), o_ptr, o_stride,
                                                           self._stream(stream)))
        return out

    def step_fused_tiled_multi_shear(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                     statistics: torch.Tensor | None = None, levels: torch.Tensor | None = None,
                                     channel_a: int = nat.STAT_Z, channel_b: int = nat.STAT_TENSION,
                                     mooring: torch.Tensor | None = None, mooring_layers: int = 1,
                                     tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                     extremes: torch.Tensor | None = None,
                                     control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                     log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                     state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                     ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_fd with the current profile set with `set_current_profile` added to the water
        (hydro_step_fused_tiled_multi_shear): the arguments and the rules are step_fused_tiled_multi_fd's, every option optional.
        Without a profile the call IS step_fused_tiled_multi_fd; with a profile and no finite-depth sea it is refused.  Returns
        the number of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_shear,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._stat_tail(n, step0, statistics, levels, channel_a, channel_b, mooring, mooring_layers, tether, layers,
                                                            peaks, extremes, control, applied, frame))

    # ------------------------------------------------------------------ seabed
    def set_seabed(self, bed) -> None:
        """The scene's floor (hydro_set_seabed; the model: include/hydro.h, "Seabed"): `bed` has `z`, `stiffness`, `damping`,
        `friction`, `slip_speed` and `friction_rate` - a `seabed.Seabed`.  None clears it.  Only `step_fused_tiled_multi_bed`
        and `seabed_wrench` see the bed.  Host-side only: the constants travel with every launch."""
        if bed is None:
            self._check(self._lib.hydro_set_seabed(self._h, None))
            self.seabed = None
            return
        c = nat.Seabed(float(bed.z), float(bed.stiffness), float(bed.damping), float(bed.friction), float(bed.slip_speed),
                       float(bed.friction_rate))
        self._check(self._lib.hydro_set_seabed(self._h, ctypes.byref(c)))
        self.seabed = bed

    def seabed_wrench(self, state: torch.Tensor, n: int, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The bed's contact wrench on each body of the tiled `state` (hydro_seabed_wrench): a tiled (tiles, 6, 64) buffer of
        [Fx Fy Fz | Tx Ty Tz], world frame, force at and torque about the body origin - exactly what a step of
        `step_fused_tiled_multi_bed` that starts from `state` adds; zeros for a body that does not touch."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.WRENCH_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
        self._check(self._lib.hydro_seabed_wrench(self._h, n, s_ptr, s_stride, o_ptr, o_stride, self._stream(stream)))
        return out

    def step_fused_tiled_multi_bed(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_sea over the seabed set with `set_seabed` (hydro_step_fused_tiled_multi_bed): in every step
        the corners of each body's box that are below the plane add a spring, damper and friction wrench, formed from the
        true state the step starts from, behind the applied wrench and the pose hold and in front of the integrator.
        control, applied, log and the sea are each optional; without a bed the call is step_fused_tiled_multi_sea.
        Returns the number of rows written (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_bed,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: (*self._applied_control(applied, frame, control, n), int(step0)))

    # ------------------------------------------------------------------ mooring lines
    def mooring_wrench(self, state: torch.Tensor, mooring: torch.Tensor, n: int, out: torch.Tensor | None = None,
                       stream=None) -> torch.Tensor:
        """The wrench of each body's mooring line on the tiled `state` (hydro_mooring_wrench; the model: include/hydro.h,
        "Mooring"): `mooring` is a tiled (tiles, 9, 64) buffer of [a(3) | b(3) | L0 | k | c] per body; the result a tiled
        (tiles, 6, 64) buffer of [Fx Fy Fz | Tx Ty Tz], world frame, force at and torque about the body origin - exactly
        what a step of `step_fused_tiled_multi_moor` that starts from `state` adds; zeros where the line adds nothing."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.WRENCH_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
        self._check(self._lib.hydro_mooring_wrench(self._h, n, s_ptr, s_stride, m_ptr, m_stride, o_ptr, o_stride,
                                                   self._stream(stream)))
        return out

    def step_fused_tiled_multi_moor(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                    mooring: torch.Tensor | None,
                                    control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                    log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                    state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                    ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_bed with one tension-only mooring line per body (hydro_step_fused_tiled_multi_moor):
        `mooring` is the tiled (tiles, 9, 64) record of `mooring_wrench`, read at every launch.  In every step a taut line
        adds a spring and damper force along itself at the fairlead, formed from the true state the step starts from,
        behind the applied wrench, the pose hold and the bed and in front of the integrator.  control, applied, log, the
        sea and the bed are each optional; mooring=None is step_fused_tiled_multi_bed.  Returns the number of rows written
        (0 without a log)."""
        def extra():
            tail = self._applied_control(applied, frame, control, n)
            m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n) if mooring is not None else (None, 0)
            return (*tail, m_ptr, m_stride, int(step0))
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_moor,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream, extra)

    # ------------------------------------------------------------------ extremes
    def extremes_reset(self, extremes: torch.Tensor, n: int, state: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Empty the tiled (tiles, 8, 64) extremes record of bodies 0 .. n - 1 (hydro_extremes_reset; the record:
        include/hydro.h, "Extremes"): [+inf, -inf] for the three position pairs, +0 for speed2_max and tension_max - or,
        with a tiled `state`, the record of that one sample, so that a run's initial state counts."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n) if state is not None else (None, 0)
        e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n)
        self._check(self._lib.hydro_extremes_reset(self._h, n, s_ptr, s_stride, e_ptr, e_stride, self._stream(stream)))
        return extremes

    def step_fused_tiled_multi_ext(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   extremes: torch.Tensor | None, mooring: torch.Tensor | None = None,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_moor that also keeps each body's running extremes (hydro_step_fused_tiled_multi_ext):
        `extremes` is the tiled (tiles, 8, 64) record of `extremes_reset`, read at the start of the launch and written at
        its end, so it accumulates over launches.  After every step the position the step produced, its squared speed and
        the line tension formed in the step enter by compare-and-select.  Nothing feeds back: states, energy and log are
        those of step_fused_tiled_multi_moor.  mooring, control, applied, log, the sea and the bed are each optional;
        extremes=None is step_fused_tiled_multi_moor.  Returns the number of rows written (0 without a log)."""
        def extra():
            tail = self._applied_control(applied, frame, control, n)
            m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n) if mooring is not None else (None, 0)
            e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n) if extremes is not None else (None, 0)
            return (*tail, m_ptr, m_stride, e_ptr, e_stride, int(step0))
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_ext,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream, extra)

    # ------------------------------------------------------------------ tethers
    def tether_wrench(self, state: torch.Tensor, tether: torch.Tensor, n: int, out: torch.Tensor | None = None,
                      tension: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The wrench of each body's tether on the tiled `state` (hydro_tether_wrench; the model: include/hydro.h,
        "Tether"): `tether` is a tiled (tiles, 7, 64) buffer of [b(3) | L0 | k | c | partner lane] per body; the result a
        tiled (tiles, 6, 64) buffer of [Fx Fy Fz | Tx Ty Tz], world frame, force at and torque about the body origin -
        exactly what a step of `step_fused_tiled_multi_teth` that starts from `state` adds; zeros where the line adds
        nothing.  `tension`, if given, is a tiled (tiles, 1, 64) buffer that receives T."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        t_ptr, t_stride = self._tiled(tether, nat.TETH_FIELDS, n)
        if out is None:
            out = self.alloc_tiled(nat.WRENCH_FIELDS, n)
        o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
        T_ptr, T_stride = self._tiled(tension, 1, n) if tension is not None else (None, 0)
        self._check(self._lib.hydro_tether_wrench(self._h, n, s_ptr, s_stride, t_ptr, t_stride, o_ptr, o_stride, T_ptr, T_stride,
                                                  self._stream(stream)))
        return out

    def step_fused_tiled_multi_teth(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                    tether: torch.Tensor | None, extremes: torch.Tensor | None = None, mooring: torch.Tensor | None = None,
                                    control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                    log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                    state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                    ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_ext with one tension-only line between two bodies of a tile (hydro_step_fused_tiled_multi_teth):
        `tether` is the tiled (tiles, 7, 64) record of `tether_wrench`, read in every step.  A taut tether adds equal and
        opposite spring and damper forces along itself at the two fairleads, formed from the true states the step starts
        from, behind the mooring line's wrench and in front of the integrator.  extremes, mooring, control, applied, log,
        the sea and the bed are each optional; tether=None is step_fused_tiled_multi_ext.  Returns the number of rows
        written (0 without a log)."""
        def extra():
            tail = self._applied_control(applied, frame, control, n)
            m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n) if mooring is not None else (None, 0)
            e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n) if extremes is not None else (None, 0)
            t_ptr, t_stride = self._tiled(tether, nat.TETH_FIELDS, n) if tether is not None else (None, 0)
            return (*tail, m_ptr, m_stride, e_ptr, e_stride, t_ptr, t_stride, int(step0))
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_teth,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream, extra)

    # ------------------------------------------------------------------ tether nets
    def _net(self, tether, layers, n):
        """(address, tile stride) of a net of `layers` tether records, a tiled (tiles, 7 * layers, 64) buffer."""
        layers = int(layers)
        if not 1 <= layers <= nat.TETH_LAYERS_MAX:
            raise ValueError(f"layers must be in 1 .. {nat.TETH_LAYERS_MAX}")
        return self._tiled(tether, nat.TETH_FIELDS * layers, n)

    def tether_net_wrench(self, state: torch.Tensor, net: torch.Tensor, n: int, layers: int, stream=None):
        """The wrench and the tension of each body's line in EACH LAYER of the net on the tiled `state`: `net` is a tiled
        (tiles, 7 * layers, 64) buffer, layer l in rows 7 l .. 7 l + 6 (include/hydro.h, "Tether net").  One call of
        hydro_tether_wrench per layer, on the layer's sub-record (the net's address + 448 l floats, the net's tile stride).
        Returns (wrenches, tensions): lists of `layers` tiled (tiles, 6, 64) and (tiles, 1, 64) buffers - what a step of
        `step_fused_tiled_multi_net` that starts from `state` adds, layer by layer; zeros where a line adds nothing."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        t_ptr, t_stride = self._net(net, layers, n)
        wrenches, tensions = [], []
        for l in range(int(layers)):
            out, tension = self.alloc_tiled(nat.WRENCH_FIELDS, n), self.alloc_tiled(1, n)
            o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
            T_ptr, T_stride = self._tiled(tension, 1, n)
            self._check(self._lib.hydro_tether_wrench(self._h, n, s_ptr, s_stride, t_ptr + 4 * nat.TETH_FIELDS * nat.TILE * l, t_stride,
                                                      o_ptr, o_stride, T_ptr, T_stride, self._stream(stream)))
            wrenches.append(out)
            tensions.append(tension)
        return wrenches, tensions

    def step_fused_tiled_multi_net(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                   tether: torch.Tensor | None, layers: int = 1, extremes: torch.Tensor | None = None,
                                   mooring: torch.Tensor | None = None,
                                   control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                   log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                   state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                   ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_teth with up to four lines per body (hydro_step_fused_tiled_multi_net): `tether` is a net,
        the tiled (tiles, 7 * layers, 64) buffer of `tether_net_wrench`, read in every step.  Every layer is a tether record
        of its own; the lines are all evaluated from the true states the step starts from and their wrenches added in
        ascending layer order.  layers=1 gives the bits of step_fused_tiled_multi_teth, tether=None those of
        step_fused_tiled_multi_ext (and `layers` is not looked at).  Returns the number of rows written (0 without a log)."""
        def extra():
            tail = self._applied_control(applied, frame, control, n)
            m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n) if mooring is not None else (None, 0)
            e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n) if extremes is not None else (None, 0)
            t_ptr, t_stride = self._net(tether, layers, n) if tether is not None else (None, 0)
            return (*tail, m_ptr, m_stride, e_ptr, e_stride, t_ptr, t_stride, int(layers), int(step0))
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_net,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream, extra)

    # ------------------------------------------------------------------ link tensions
    def step_fused_tiled_multi_peak(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                    tether: torch.Tensor | None, layers: int = 1, peaks: torch.Tensor | None = None,
                                    extremes: torch.Tensor | None = None, mooring: torch.Tensor | None = None,
                                    control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                    log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                    state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                    ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_net that also keeps the PEAK TENSION of every line (hydro_step_fused_tiled_multi_peak; the
        record: include/hydro.h, "Link tensions"): `peaks` is a tiled (tiles, layers, 64) buffer, row l the running maximum of
        each body's line in layer l of the net - updated in every step where the line pulls, never reset by a launch (zero it
        to start over), so it accumulates over launches.  Nothing feeds back: states, energy, log and extremes are the bits
        of step_fused_tiled_multi_net.  peaks=None IS that call.  Returns the number of rows written (0 without a log)."""
        def extra():
            tail = self._applied_control(applied, frame, control, n)
            m_ptr, m_stride = self._tiled(mooring, nat.MOOR_FIELDS, n) if mooring is not None else (None, 0)
            e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n) if extremes is not None else (None, 0)
            t_ptr, t_stride = self._net(tether, layers, n) if tether is not None else (None, 0)
            p_ptr, p_stride = self._tiled(peaks, int(layers), n) if peaks is not None else (None, 0)
            return (*tail, m_ptr, m_stride, e_ptr, e_stride, t_ptr, t_stride, int(layers), p_ptr, p_stride, int(step0))
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_peak,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream, extra)

    # ------------------------------------------------------------------ mooring spreads
    def _spread(self, spread, layers, n):
        """(address, tile stride) of a spread of `layers` mooring records, a tiled (tiles, 9 * layers, 64) buffer."""
        layers = int(layers)
        if not 1 <= layers <= nat.MOOR_LAYERS_MAX:
            raise ValueError(f"mooring_layers must be in 1 .. {nat.MOOR_LAYERS_MAX}")
        return self._tiled(spread, nat.MOOR_FIELDS * layers, n)

    def mooring_spread_wrench(self, state: torch.Tensor, spread: torch.Tensor, n: int, layers: int, stream=None) -> list:
        """The wrench of each body's line in EACH LAYER of the spread on the tiled `state`: `spread` is a tiled
        (tiles, 9 * layers, 64) buffer, layer l in rows 9 l .. 9 l + 8 (include/hydro.h, "Mooring spread").  One call of
        hydro_mooring_wrench per layer, on the layer's sub-record (the spread's address + 576 l floats, the spread's tile
        stride).  Returns a list of `layers` tiled (tiles, 6, 64) buffers - what a step of `step_fused_tiled_multi_spread`
        that starts from `state` adds, layer by layer; zeros where a line adds nothing."""
        s_ptr, s_stride = self._tiled(state, nat.STATE_FIELDS, n)
        m_ptr, m_stride = self._spread(spread, layers, n)
        wrenches = []
        for l in range(int(layers)):
            out = self.alloc_tiled(nat.WRENCH_FIELDS, n)
            o_ptr, o_stride = self._tiled(out, nat.WRENCH_FIELDS, n)
            self._check(self._lib.hydro_mooring_wrench(self._h, n, s_ptr, s_stride, m_ptr + 4 * nat.MOOR_FIELDS * nat.TILE * l, m_stride,
                                                       o_ptr, o_stride, self._stream(stream)))
            wrenches.append(out)
        return wrenches

    def step_fused_tiled_multi_spread(self, state: torch.Tensor, prev_state: torch.Tensor, n: int, dt: float, steps: int, step0: int,
                                      mooring: torch.Tensor | None, mooring_layers: int = 1,
                                      tether: torch.Tensor | None = None, layers: int = 1, peaks: torch.Tensor | None = None,
                                      extremes: torch.Tensor | None = None,
                                      control: torch.Tensor | None = None, applied: torch.Tensor | None = None, frame: str = "body",
                                      log: torch.Tensor | None = None, every: int = 1, phase: int = 1, row0: int = 0,
                                      state_out: torch.Tensor | None = None, implicit_drag: bool = False, stream=None,
                                      ke_out: torch.Tensor | None = None, rotational: bool = True) -> int:
        """step_fused_tiled_multi_peak with up to four anchored lines per body (hydro_step_fused_tiled_multi_spread): `mooring`
        is a spread, the tiled (tiles, 9 * mooring_layers, 64) buffer of `mooring_spread_wrench`, read in every step.  Every
        layer is a mooring record of its own; the lines are all evaluated from the true state the step starts from and their
        wrenches added in ascending layer order, behind the bed and in front of the tethers; `tension_max` of the extremes
        takes the largest tension of a body's lines.  mooring_layers=1 gives the bits of step_fused_tiled_multi_peak with the
        same record, mooring=None IS that call (and `mooring_layers` is not looked at).  Returns the number of rows written
        (0 without a log)."""
        return self._recorded_multi(self._lib.hydro_step_fused_tiled_multi_spread,
                                    (state, prev_state, n, dt, steps, state_out, implicit_drag, ke_out, rotational),
                                    (log, every, phase, row0), stream,
                                    lambda: self._spread_tail(n, step0, mooring, mooring_layers, tether, layers, peaks, extremes, control, applied, frame))

    def _spread_tail(self, n, step0, mooring, mooring_layers, tether, layers, peaks, extremes, control, applied, frame):
        """The arguments `applied .. step0` of `hydro_step_fused_tiled_multi_spread` / `_irr`: every buffer may be None (NULL, stride 0)."""
        tail = self._applied_control(applied, frame, control, n)
        m_ptr, m_stride = self._spread(mooring, mooring_layers, n) if mooring is not None else (None, 0)
        e_ptr, e_stride = self._tiled(extremes, nat.EXT_FIELDS, n) if extremes is not None else (None, 0)
        t_ptr, t_stride = self._net(tether, layers, n) if tether is not None else (None, 0)
        p_ptr, p_stride = self._tiled(peaks, int(layers), n) if peaks is not None else (None, 0)
        return (*tail, m_ptr, m_stride, int(mooring_layers), e_ptr, e_stride, t_ptr, t_stride, int(layers), p_ptr, p_stride, int(step0))

    def integrate_tiled(self, state_in: torch.Tensor, wrench: torch.Tensor, n: int, dt: float,
                        state_out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if state_out is None:
            state_out = torch.zeros_like(state_in)
        ins = self._tiled(state_in, nat.STATE_FIELDS, n) + self._tiled(wrench, nat.WRENCH_FIELDS, n)
        self._check(self._lib.hydro_integrate_tiled(self._h, n, *ins, float(dt), *self._tiled(state_out, nat.STATE_FIELDS, n),
                                                    self._stream(stream)))
        return state_out

    # ------------------------------------------- simulator tensors (array of structs)
    def _rows(self, tensors, widths, n: int, what: str = "tensor") -> None:
        """Each of `tensors` must be a contiguous float32 (n, width) tensor on the engine's device."""
        for t, w in zip(tensors, widths):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != (n, w) or t.device != self.device:
                raise ValueError(f"expected contiguous float32 ({n},{w}) {what} on {self.device}")

    def _force_torque(self, n: int, forces, torques):
        """The (n,3) outputs of an array-of-structs entry, allocated where None (given ones are taken as they are)."""
        if forces is None:
            forces = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        if torques is None:
            torques = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        return forces, torques

    def pack_state_aos(self, positions: torch.Tensor, orientations: torch.Tensor, velocities: torch.Tensor,
                       out: torch.Tensor | None = None, quat_xyzw: bool = False, stream=None) -> torch.Tensor:
        """Simulator tensors (N,3), (N,4), (N,6) -> tiled state (tiles,13,64)."""
        n = positions.shape[0]
        if out is None:
            out = self.alloc_tiled(nat.STATE_FIELDS, n)
        self._check(self._lib.hydro_pack_state_aos(
            self._h, n, positions.data_ptr(), orientations.data_ptr(), int(bool(quat_xyzw)), velocities.data_ptr(),
            *self._tiled(out, nat.STATE_FIELDS, n), self._stream(stream)))
        return out

    def unpack_wrench_aos(self, wrench: torch.Tensor, n: int, forces: torch.Tensor | None = None,
                          torques: torch.Tensor | None = None, stream=None):
        w = self._tiled(wrench, nat.WRENCH_FIELDS, n)
        forces, torques = self._force_torque(n, forces, torques)
        self._check(self._lib.hydro_unpack_wrench_aos(self._h, n, *w, forces.data_ptr(), torques.data_ptr(),
                                                      self._stream(stream)))
        return forces, torques

    def _wrench_aos_call(self, positions, orientations, velocities, forces, torques, quat_xyzw):
        """The arguments of `hydro_step_wrench_aos` before and after `dt` (the stream follows) and the outputs: the three
        inputs validated, `forces` / `torques` allocated where None."""
        n = positions.shape[0]
        self._rows((positions, orientations, velocities), (3, 4, 6), n)
        forces, torques = self._force_torque(n, forces, torques)
        head = (self._h, n, positions.data_ptr(), orientations.data_ptr(), int(bool(quat_xyzw)), velocities.data_ptr())
        return head, (forces.data_ptr(), torques.data_ptr()), forces, torques

    def step_wrench_aos(self, positions: torch.Tensor, orientations: torch.Tensor, velocities: torch.Tensor,
                        dt: float, forces: torch.Tensor | None = None, torques: torch.Tensor | None = None,
                        quat_xyzw: bool = False, stream=None):
        """Fused wrench on the simulator's tensors: positions (N,3), orientations (N,4) (WXYZ as the
        simulator gives them, or XYZW with quat_xyzw=True), velocities (N,6) -> forces (N,3),
        torques (N,3).  Uses and updates the engine's previous-velocity state."""
        head, tail, forces, torques = self._wrench_aos_call(positions, orientations, velocities, forces, torques, quat_xyzw)
        self._check(self._lib.hydro_step_wrench_aos(*head, float(dt), *tail, self._stream(stream)))
        return forces, torques

    def step_wrench_aos_sea(self, positions: torch.Tensor, orientations: torch.Tensor, velocities: torch.Tensor,
                            dt: float, time: float, forces: torch.Tensor | None = None, torques: torch.Tensor | None = None,
                            quat_xyzw: bool = False, stream=None):
        """`step_wrench_aos` through the sea set with `set_sea`, at `time` seconds (hydro_step_wrench_aos_sea).  The engine's
        previous-velocity state receives the TRUE velocity.  Without a sea the call is step_wrench_aos."""
        head, tail, forces, torques = self._wrench_aos_call(positions, orientations, velocities, forces, torques, quat_xyzw)
        self._check(self._lib.hydro_step_wrench_aos_sea(*head, float(dt), *tail, float(time), self._stream(stream)))
        return forces, torques

    def step_wrench_aos_irr(self, positions: torch.Tensor, orientations: torch.Tensor, velocities: torch.Tensor,
                            dt: float, time: float, forces: torch.Tensor | None = None, torques: torch.Tensor | None = None,
                            quat_xyzw: bool = False, stream=None):
        """`step_wrench_aos_sea` through whichever sea the engine holds, at `time` seconds (hydro_step_wrench_aos_irr): a
        finite-depth sea, an ensemble, a spectrum, or the sea of `set_sea`.  The engine's previous-velocity state receives the
        TRUE velocity.  Without any sea the call is step_wrench_aos."""
        head, tail, forces, torques = self._wrench_aos_call(positions, orientations, velocities, forces, torques, quat_xyzw)
        self._check(self._lib.hydro_step_wrench_aos_irr(*head, float(dt), *tail, float(time), self._stream(stream)))
        return forces, torques

    def prepare_step_wrench_aos(self, positions: torch.Tensor, orientations: torch.Tensor, velocities: torch.Tensor,
                                forces: torch.Tensor | None = None, torques: torch.Tensor | None = None,
                                quat_xyzw: bool = False):
        """Build the launch of `step_wrench_aos` ONCE (`_wrench_aos_call`; given outputs are validated here as well) and
        return `step(dt, stream=None, time=None) -> (forces, torques)`, which re-issues that launch on the same buffers (a
        simulator's tensor API hands out views of the same device buffers every physics step).  For the plugin path,
        where the per-call Python work of `step_wrench_aos` (tensor checks, pointer conversions) is several times the
        kernel at 20 bodies.  `time` None: `hydro_step_wrench_aos`, argument for argument; otherwise the `_sea` entry at
        `time` seconds - the `_irr` entry while the engine holds a spectrum, an ensemble or a finite-depth sea
        (`holds_irregular_sea`, asked at every step).  `stream`: a torch stream / raw handle; None = the stream current at the time of the call."""
        head, tail, forces, torques = self._wrench_aos_call(positions, orientations, velocities, forces, torques, quat_xyzw)
        self._rows((forces, torques), (3, 3), positions.shape[0], "output")
        head, tail = _prebuilt("hydro_step_wrench_aos", head), _prebuilt("hydro_step_wrench_aos", tail, len(head) + 1)
        fn, sea_fn, check = self._lib.hydro_step_wrench_aos, self._lib.hydro_step_wrench_aos_sea, self._check
        irr_fn, irregular = self._lib.hydro_step_wrench_aos_irr, self.holds_irregular_sea
        keep = (positions, orientations, velocities, forces, torques)          # the buffers must outlive the callable
        dev, cur = self.device, torch.cuda.current_stream
        # the current stream's raw handle without building a torch.cuda.Stream object (0.2 instead of 1 us per step)
        raw_current, dev_index = getattr(torch._C, "_cuda_getCurrentRawStream", None), self.device.index
        last = [None, None]                              # (dt, its c_double): a simulator steps with ONE dt

        def step(dt: float, stream=None, time=None):          # (stream stays the second positional argument)
            if self._h is None:
                raise HydroError(nat.HYDRO_E_STATE, "engine is closed")
            if stream is None:
                sp = raw_current(dev_index) if raw_current is not None else cur(dev).cuda_stream
            else:
                sp = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
            if dt != last[0]:
                last[0], last[1] = dt, ctypes.c_double(dt)
            if time is None:
                rc = fn(*head, last[1], *tail, sp)
            else:
                rc = (irr_fn if irregular() else sea_fn)(*head, last[1], *tail, ctypes.c_double(time), sp)
            if rc:
                check(rc)
            return keep[3], keep[4]
        return step

    def step_components(self, state: torch.Tensor, accel: torch.Tensor, out: torch.Tensor | None = None,
                        ratio: torch.Tensor | None = None, stream=None):
        """Component mode: state (13,N), accel (6,N) -> comps (24,N), ratio (N,)."""
        n = state.shape[1]
        if out is None:
            out = torch.empty((nat.COMP_FIELDS, n), dtype=torch.float32, device=self.device)
        if ratio is None:
            ratio = torch.empty((n,), dtype=torch.float32, device=self.device)
        self._check(self._lib.hydro_step_components(
            self._h, n, self._table(state, nat.STATE_FIELDS), self._table(accel, nat.PREV_FIELDS),
            self._table(out, nat.COMP_FIELDS), ratio.data_ptr(), self._stream(stream)))
        return out, ratio

    def step_components_aos(self, position, orientation_xyzw, linear_vel, angular_vel, linear_accel, angular_accel,
                            out: torch.Tensor, ratio: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Component mode on the calculator's argument layout: (N,3)/(N,4) tensors in, out (8,N,3)."""
        n = position.shape[0]
        ins = (position, orientation_xyzw, linear_vel, angular_vel, linear_accel, angular_accel)
        self._rows(ins, (3, 4, 3, 3, 3, 3), n)
        if out.shape != (8, n, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"expected contiguous float32 (8,{n},3) output on {self.device}")
        key = ("comp_aos", out.data_ptr(), n)
        tab = self._tables.get(key)
        if tab is None:
            tab = self._tables[key] = nat.pointer_table([out.data_ptr() + k * n * 12 for k in range(8)])
        self._check(self._lib.hydro_step_components_aos(
            self._h, n, *[t.data_ptr() for t in ins], tab, ratio.data_ptr() if ratio is not None else None,
            self._stream(stream)))
        return out

    def kinetic_energy(self, state: torch.Tensor, rotational: bool = False, out: torch.Tensor | None = None,
                       stream=None) -> torch.Tensor:
        """[sum 1/2 m v^2, sum 1/2 w.I.w] as a float64 device tensor of shape (2,)."""
        if out is None:
            out = torch.empty((2,), dtype=torch.float64, device=self.device)
        if state.ndim == 3:                       # tiled (tiles,13,64): n = bodies with parameters set
            self._check(self._lib.hydro_kinetic_energy_tiled(self._h, self.n, *self._tiled(state, nat.STATE_FIELDS, self.n),
                                                             int(bool(rotational)), out.data_ptr(), self._stream(stream)))
            return out
        self._check(self._lib.hydro_kinetic_energy(self._h, state.shape[1], self._table(state, nat.STATE_FIELDS),
                                                   int(bool(rotational)), out.data_ptr(), self._stream(stream)))
        return out

    def ke_allreduce(self, nccl_comm: int, ke: torch.Tensor, stream=None) -> torch.Tensor:
        """Sum the pair a kinetic-energy entry left in `ke` over the ranks of an RCCL communicator (raw ncclComm_t
        address), in place, on `stream` (hydro_ke_allreduce: the C-level route; the Python monitor of simulate.py uses
        torch.distributed for the same collective)."""
        self._check_ke_out(ke)
        self._check(self._lib.hydro_ke_allreduce(self._h, ctypes.c_void_p(nccl_comm), ke.data_ptr(), self._stream(stream)))
        return ke

    def ke_rearm(self, stream=None) -> None:
        """Zero the ticket counters of the kinetic-energy reduction on `stream` (hydro_ke_rearm): the recovery path after
        a launch that did not run to its end - such a launch leaves NaNs in its output, never a stale pair."""
        self._check(self._lib.hydro_ke_rearm(self._h, self._stream(stream)))

    @staticmethod
    def bind_rccl(library: "ctypes.CDLL | str | None") -> str:
        """Tell hydro_ke_allreduce which RCCL to call: the ctypes library object (or path) of the copy that made the
        communicators - a communicator belongs to ONE loaded copy.  None forgets the binding.  Returns
        hydro_rccl_origin()."""
        lib = nat.load()
        if library is None:
            lib.hydro_bind_rccl(None, None)
        else:
            rccl = ctypes.CDLL(library) if isinstance(library, str) else library
            err = ctypes.cast(rccl.ncclGetErrorString, ctypes.c_void_p) if hasattr(rccl, "ncclGetErrorString") else None
            lib.hydro_bind_rccl(ctypes.cast(rccl.ncclAllReduce, ctypes.c_void_p), err)
        return lib.hydro_rccl_origin().decode()

    def integrate(self, state_in: torch.Tensor, wrench: torch.Tensor, dt: float,
                  state_out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if state_out is None:
            state_out = torch.empty_like(state_in)
        self._check(self._lib.hydro_integrate(
            self._h, state_in.shape[1], self._table(state_in, nat.STATE_FIELDS), self._table(wrench, nat.WRENCH_FIELDS),
            float(dt), self._table(state_out, nat.STATE_FIELDS), self._stream(stream)))
        return state_out

    # ----------------------------------------------------------------- lifetime
    def sync(self) -> None:
        self._check(self._lib.hydro_sync(self._h))
        torch.cuda.current_stream(self.device).synchronize()

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.hydro_destroy(self._h)
            self._h = None
            self._tables.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
