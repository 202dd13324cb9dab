"""Stand-ins that let the Python host run without a GPU: a fake libhydro that records `(name, argument values)` for every
`hydro_*` call and returns 0, tensors with chosen addresses (tests/test_engine_calls.py explains the conventions), and fake engines
that record the calls ClosedLoopSim makes.  Used by the CPU tests of every resident option.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import simulate
from silver2_isaacsim_amd.engine import HydroEngine
from silver2_isaacsim_amd.sea import SeaState
from silver2_isaacsim_amd.seabed import Seabed

DEV = torch.device("cuda:0")
HANDLE = 0xABC000                 # engine k of a test gets HANDLE + 0x100 * k
STREAM = 0x5700
N, TILES = 1000, 16               # ceil(1000 / 64)
DT = 0.01


class T:
    """What the host reads of a tensor: data_ptr / shape / dtype / device / ndim / dim / numel / is_contiguous."""

    def __init__(self, shape, ptr, dtype=torch.float32, device=DEV, contiguous=True):
        self.shape, self._ptr, self.dtype, self.device, self._contiguous = tuple(shape), ptr, dtype, device, contiguous

    ndim = property(lambda self: len(self.shape))

    def dim(self):
        return len(self.shape)

    def numel(self):
        k = 1
        for s in self.shape:
            k *= s
        return k

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._ptr


def plain(a):
    """An argument as the C side would see it: ctypes scalars -> their value, arrays and structs -> tuples."""
    if isinstance(a, ctypes.Array):
        return tuple(plain(x) for x in a)
    if isinstance(a, ctypes.Structure):
        return tuple(plain(getattr(a, name)) for name, _ in a._fields_)
    if hasattr(a, "_obj"):                                   # ctypes.byref(x)
        return ("byref", plain(a._obj))
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    return a


class FakeLib:
    def __init__(self):
        self.calls, self.created = [], 0

    def __getattr__(self, name):
        if not name.startswith("hydro_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "hydro_create":
                args[2]._obj.value = HANDLE + 0x100 * self.created
                self.created += 1
            self.calls.append((name, tuple(plain(a) for a in args)))
            return 0
        return fn


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(nat, "_lib", fake)
    return fake


def make_engine(lib, n=N):
    eng = HydroEngine(1000, "cuda:0")
    eng.n = n                                                # what set_params would leave
    lib.calls.clear()
    return eng


@pytest.fixture
def eng(lib):
    return make_engine(lib)


# the stand-ins: one address each, far enough apart that no offset of one reaches another
S = T((TILES, 13, 64), 0x10000000)
P6 = T((TILES, 6, 64), 0x20000000)
P13 = T((TILES, 13, 64), 0x30000000)
O = T((TILES, 6, 64), 0x40000000)
SO = T((TILES, 13, 64), 0x50000000)
KE = T((2,), 0x60000000, dtype=torch.float64)
POS, ORI, VELS = T((N, 3), 0x70000000), T((N, 4), 0x71000000), T((N, 6), 0x72000000)
F, TQ = T((N, 3), 0x73000000), T((N, 3), 0x74000000)
PREVS = [(None, (None, 0)), (P6, (0x20000000, 384)), (P13, (0x30000000 + 1792, 832))]
H = HANDLE


def refused(lib, msg, fn, *a, **kw):
    with pytest.raises(ValueError) as ei:
        fn(*a, **kw)
    assert str(ei.value) == msg
    assert lib.calls == []


FUSED_HEAD = (H, 1000, 0x10000000, 832, 0x30000000 + 1792, 832, 0.01)
BED = Seabed(-25.0, 144.0, 2.4, 0.5, 0.01, 2.4)


class FakeEngine:
    """Records the calls ClosedLoopSim makes; nothing runs.  alloc_tiled gives a host tensor."""

    def __init__(self):
        self.calls = []

    def alloc_tiled(self, fields, n):
        return torch.zeros(((n + 63) // 64, fields, 64), dtype=torch.float32)

    def set_seabed(self, bed):
        self.calls.append(("set_seabed", bed))

    def _step(self, name, cur, steps, **kw):
        self.calls.append(dict(method=name, cur=cur, steps=steps, **kw))
        return 0

    def step_fused_tiled_multi_moor(self, cur, old, n, dt, steps, step0, mooring, control, applied, frame, implicit_drag=False, ke_out=None,
                                    log=None, **rec):
        return self._step("moor", cur, steps, step0=step0, mooring=mooring, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_bed(self, cur, old, n, dt, steps, step0, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("bed", cur, steps, step0=step0, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_sea(self, cur, old, n, dt, steps, step0, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("sea", cur, steps, step0=step0, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_controlled(self, cur, old, n, dt, steps, control, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("ctl", cur, steps, control=control, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_applied(self, cur, old, n, dt, steps, applied, frame, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("app", cur, steps, applied=applied, frame=frame, log=log)

    def step_fused_tiled_multi_rec(self, cur, old, n, dt, steps, implicit_drag=False, ke_out=None, log=None, **rec):
        return self._step("rec", cur, steps, log=log)

    def step_fused_tiled_multi(self, cur, old, n, dt, steps, **kw):
        self._step("plain", cur, steps)

    def step_fused_tiled(self, cur, old, n, dt, **kw):
        self._step("single", cur, None)


class _Ctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


BODIES = 70                                                        # two tiles


def moor_sim(monkeypatch, recorder=False, applied=False, control=False, sea=False, bed=False):
    monkeypatch.setattr(simulate.torch.cuda, "stream", lambda s: _Ctx())
    s = object.__new__(simulate.ClosedLoopSim)
    s.fused, s.implicit_drag, s.n, s.dt, s.engine = True, True, BODIES, 1.0 / 60.0, FakeEngine()
    params = np.zeros((BODIES, 11), np.float32)
    params[:, 10] = 500.0
    s.scene = types.SimpleNamespace(params=params)
    s.cur, s.old, s.stream = "buffer A", "buffer B", None
    s.steps_done, s.monitor, s._monitor_warm, s.ke_dev = 0, None, True, None
    s.recorder = simulate.TrajectoryRecorder([5, 2], every=2, rows=64, sim=s) if recorder else None
    s.applied, s.applied_frame = ("the applied buffer" if applied else None), "world"
    s.control = "the control buffer" if control else None
    s.sea = SeaState((0.3, 0.0, 0.0)) if sea else None
    if bed:
        s.seabed = BED
    s._graph, s._graph_steps, s._graph_bufs = None, 0, None
    s.synchronize = lambda timeout_s=None: None
    return s


LINES = dict(anchor=[[1.0, 2.0, -20.0], [3.0, 4.0, -21.0]], fairlead=(0.0, 0.1, -0.5), length=[19.0, 20.0], stiffness=7200.0, damping=600.0,
             bodies=[66, 3])


# what the sim calls without lines, by the rule of tests/test_sim_dispatch.py and tests/test_seabed.py
def _without_lines(recorder, applied, control, sea, bed, eager):
    return "bed" if bed else "sea" if sea else "ctl" if control else "app" if applied else "rec" if recorder else "single" if eager else "plain"


class ExtEngine(FakeEngine):
    """FakeEngine with the two calls of the extremes."""

    def extremes_reset(self, extremes, n, state=None, stream=None):
        self.calls.append(("extremes_reset", extremes, n, state))
        return extremes

    def step_fused_tiled_multi_ext(self, cur, old, n, dt, steps, step0, extremes, mooring, control, applied, frame, implicit_drag=False, ke_out=None,
                                   log=None, **rec):
        return self._step("ext", cur, steps, step0=step0, extremes=extremes, mooring=mooring, control=control, applied=applied, frame=frame, log=log)


def ext_sim(monkeypatch, recorder=False, applied=False, control=False, sea=False, bed=False, lines=False):
    s = moor_sim(monkeypatch, recorder, applied, control, sea, bed)
    s.engine = ExtEngine()
    if lines:
        s.set_mooring(**LINES)
    return s


def _without_extremes(recorder, applied, control, sea, bed, lines, eager):
    return "moor" if lines else _without_lines(recorder, applied, control, sea, bed, eager)
