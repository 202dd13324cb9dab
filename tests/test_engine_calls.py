"""The Python host's marshalling, without a GPU: which C function every `HydroEngine` method calls and with which
argument values, and which inputs it refuses with which message.

`_native._lib` is replaced by a fake that records `(name, argument values)` for every `hydro_*` call and returns 0, so
`HydroEngine(1000, "cuda:0")` constructs on any machine.  Tensors are small stand-ins with chosen addresses; every case
passes each output buffer and the stream explicitly, so nothing allocates on a device and nothing asks torch for the
current stream.  Expected values are literals or arithmetic on the stand-ins' addresses (a 13-field state tile is
13 * 64 = 832 floats, a 6-field tile 384, the velocity fields start 7 * 64 * 4 = 1792 bytes into a state tile) - never
the output of the code under test.  ctypes values and plain Python values count as the same argument: the prepared
forms pass the former, the direct ones may pass either.
"""

import pytest
import torch

from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd.engine import HydroEngine
from engine_stand_ins import (DEV, DT, eng, F, FUSED_HEAD, H, HANDLE, KE, lib, make_engine, N, O, ORI, P13, P6, POS, PREVS, refused, S, SO, STREAM, T, TILES, TQ,
                              VELS)  # noqa: F401  (fixtures are requested by name)

VEL = 7 * 64 * 4                  # byte offset of vx inside a state tile
ST, WR = 13 * 64, 6 * 64          # tile strides, in floats


RATIO = T((N,), 0x75000000)


def table(t):
    """Field pointers of a plain (F, n) float32 stand-in."""
    return tuple(t.data_ptr() + f * t.shape[1] * 4 for f in range(t.shape[0]))


def test_construction_and_constants(lib):
    eng = HydroEngine(1000, "cuda:0", 1000.0, 9.8)
    assert lib.calls == [("hydro_create", (0, 1000, ("byref", H))), ("hydro_set_scene", (H, 1000.0, 9.8))]
    assert eng.device == DEV and eng.capacity == 1000 and eng.n == 0
    assert (nat.TILE, nat.STATE_FIELDS, nat.PREV_FIELDS, nat.WRENCH_FIELDS) == (64, 13, 6, 6)
    assert nat.STATUS_NAMES == {0: "HYDRO_OK", -1: "HYDRO_E_ARG", -2: "HYDRO_E_ALLOC", -3: "HYDRO_E_LAUNCH",
                                -4: "HYDRO_E_DEVICE", -5: "HYDRO_E_STATE"}


# ------------------------------------------------------------------------------------------------ tiled wrench
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("prev,prev_args", PREVS)
def test_step_wrench_tiled(lib, eng, prev, prev_args, prepared):
    head = (H, 1000, 0x10000000, 832) + prev_args + (0.01, 0x40000000, 384)
    cases = [(dict(), ("hydro_step_wrench_tiled", head + (STREAM,))),
             (dict(rotational=False), ("hydro_step_wrench_tiled", head + (STREAM,))),
             (dict(ke_out=KE), ("hydro_step_wrench_tiled_ke", head + (1, 0x60000000, STREAM))),
             (dict(ke_out=KE, rotational=False), ("hydro_step_wrench_tiled_ke", head + (0, 0x60000000, STREAM)))]
    for kw, want in cases:
        lib.calls.clear()
        if prepared:
            step = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=prev, stream=STREAM, **kw)
            assert lib.calls == []                           # preparing launches nothing
            assert step() is O and step() is O
            assert lib.calls == [want, want]
        else:
            assert eng.step_wrench_tiled(S, N, DT, out=O, prev=prev, stream=STREAM, **kw) is O
            assert lib.calls == [want]


def test_step_wrench_tiled_positional_order(lib, eng):
    """(state, n, dt, out, prev, stream, ke_out, rotational) for both forms."""
    want = ("hydro_step_wrench_tiled_ke", (H, 1000, 0x10000000, 832, 0x20000000, 384, 0.01, 0x40000000, 384, 0,
                                           0x60000000, STREAM))
    eng.step_wrench_tiled(S, N, DT, O, P6, STREAM, KE, False)
    eng.prepare_step_wrench_tiled(S, N, DT, O, P6, STREAM, KE, False)()
    assert lib.calls == [want, want]


def test_fewer_bodies_than_the_buffers_hold(lib, eng):
    eng.step_wrench_tiled(S, 100, 0.5, out=O, prev=P13, stream=STREAM)
    assert lib.calls == [("hydro_step_wrench_tiled", (H, 100, 0x10000000, 832, 0x30000000 + 1792, 832, 0.5,
                                                      0x40000000, 384, STREAM))]


def test_stream_objects_and_raw_handles(lib, eng):
    class Stream:
        cuda_stream = 0x7700
    eng.step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=Stream())
    eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=Stream())()
    assert [c[1][-1] for c in lib.calls] == [0x7700, 0x7700]


def test_prepared_callables_on_a_closed_engine(lib, eng):
    tiled = eng.prepare_step_wrench_tiled(S, N, DT, out=O, prev=P6, stream=STREAM)
    aos = eng.prepare_step_wrench_aos(POS, ORI, VELS, F, TQ)
    eng.close()
    assert lib.calls == [("hydro_destroy", (H,))]
    for call in (tiled, lambda: aos(DT, STREAM)):
        with pytest.raises(nat.HydroError) as ei:
            call()
        assert ei.value.status == -5 and str(ei.value) == "HYDRO_E_STATE: engine is closed"
    assert len(lib.calls) == 1


# ------------------------------------------------------------------------------------------------------- batch
def test_prepare_step_wrench_tiled_batch(lib):
    e1, e2 = make_engine(lib, 1000), make_engine(lib, 130)   # 130 bodies: 3 tiles
    h1, h2 = HANDLE, HANDLE + 0x100
    s2, o2 = T((3, 13, 64), 0x11000000), T((3, 6, 64), 0x41000000)
    p2 = T((3, 13, 64), 0x31000000)
    outs = [O, o2]
    step, got = HydroEngine.prepare_step_wrench_tiled_batch([e1, e2], [S, s2], DT, outs=outs, prevs=[P6, p2], stream=STREAM)
    assert lib.calls == [] and got == outs
    assert step() == outs
    assert lib.calls == [("hydro_step_wrench_tiled_batch", (2, (
        (h1, 1000, 0x10000000, 832, 0x20000000, 384, 0x40000000, 384),
        (h2, 130, 0x11000000, 832, 0x31000000 + 1792, 832, 0x41000000, 384)), 0.01, STREAM))]
    lib.calls.clear()
    step(stream=0x7700)                                      # the stream may be given per call
    assert lib.calls[0][1][3] == 0x7700

    lib.calls.clear()                                        # engine-owned previous velocities, explicit body counts
    got = HydroEngine.step_wrench_tiled_batch([e2, e1], [s2, S], 0.25, outs=[o2, O], prevs=None, ns=[70, 999], stream=STREAM)
    assert got == [o2, O]
    assert lib.calls == [("hydro_step_wrench_tiled_batch", (2, (
        (h2, 70, 0x11000000, 832, None, 0, 0x41000000, 384),
        (h1, 999, 0x10000000, 832, None, 0, 0x40000000, 384)), 0.25, STREAM))]


def test_batch_refusals(lib, eng):
    msg = "1 .. 32 scenes per launch, one state buffer each"
    refused(lib, msg, HydroEngine.prepare_step_wrench_tiled_batch, [], [], DT)
    refused(lib, msg, HydroEngine.prepare_step_wrench_tiled_batch, [eng] * 33, [S] * 33, DT, outs=[O] * 33, stream=STREAM)
    refused(lib, msg, HydroEngine.prepare_step_wrench_tiled_batch, [eng, eng], [S], DT, outs=[O, O], stream=STREAM)
    tiled = "expected contiguous float32 (>= 16, {}, 64) tensor on cuda:0"
    batch = HydroEngine.prepare_step_wrench_tiled_batch
    refused(lib, tiled.format(13), batch, [eng], [P6], DT, outs=[O], stream=STREAM)
    refused(lib, tiled.format(6), batch, [eng], [S], DT, outs=[S], stream=STREAM)
    refused(lib, tiled.format(6), batch, [eng], [S], DT, outs=[O], prevs=[T((TILES, 5, 64), 0x1000)], stream=STREAM)
    refused(lib, tiled.format(13), batch, [eng], [S], DT, outs=[O], prevs=[T((TILES - 1, 13, 64), 0x1000)], stream=STREAM)
    # 32 scenes are taken
    step, _ = batch([eng] * 32, [S] * 32, DT, outs=[O] * 32, stream=STREAM)
    step()
    assert lib.calls[0][1][0] == 32 and len(lib.calls[0][1][1]) == 32


# ------------------------------------------------------------------------------------------------------- fused


@pytest.mark.parametrize("state_out,so_ptr", [(SO, 0x50000000), (None, 0x30000000)])
@pytest.mark.parametrize("wrench,w_args", [(None, (None, 0)), (O, (0x40000000, 384))])
def test_step_fused_tiled(lib, eng, state_out, so_ptr, wrench, w_args):
    ret = P13 if state_out is None else SO
    mid = (so_ptr, 832) + w_args
    cases = [(dict(), ("hydro_step_fused_tiled", FUSED_HEAD + mid + (0, STREAM))),
             (dict(implicit_drag=True, rotational=False), ("hydro_step_fused_tiled", FUSED_HEAD + mid + (1, STREAM))),
             (dict(ke_out=KE), ("hydro_step_fused_tiled_ke", FUSED_HEAD + mid + (0, 1, 0x60000000, STREAM))),
             (dict(ke_out=KE, implicit_drag=True, rotational=False),
              ("hydro_step_fused_tiled_ke", FUSED_HEAD + mid + (1, 0, 0x60000000, STREAM)))]
    for kw, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled(S, P13, N, DT, state_out=state_out, wrench=wrench, stream=STREAM, **kw) is ret
        assert lib.calls == [want]


@pytest.mark.parametrize("state_out,so_ptr", [(SO, 0x50000000), (None, 0x30000000)])
def test_step_fused_tiled_multi(lib, eng, state_out, so_ptr):
    ret = P13 if state_out is None else SO
    mid = (so_ptr, 832, 0x10000000 + 1792, 832)
    cases = [(dict(), FUSED_HEAD + (5,) + mid + (0, 1, None, STREAM)),
             (dict(implicit_drag=True, rotational=False), FUSED_HEAD + (5,) + mid + (1, 0, None, STREAM)),
             (dict(ke_out=KE), FUSED_HEAD + (5,) + mid + (0, 1, 0x60000000, STREAM)),
             (dict(ke_out=KE, implicit_drag=True, rotational=False), FUSED_HEAD + (5,) + mid + (1, 0, 0x60000000, STREAM))]
    for kw, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi(S, P13, N, DT, 5, state_out=state_out, stream=STREAM, **kw) is ret
        assert lib.calls == [("hydro_step_fused_tiled_multi", want)]


@pytest.mark.parametrize("fields", [13, 19])
def test_step_fused_tiled_multi_rec(lib, eng, fields):
    log = T((10, fields, 8), 0x80000000)
    mid = (0x10000000 + 1792, 832)
    rec = (0x80000000, 8, 10, fields, 4, 1, 2, ("byref", 0), STREAM)
    cases = [(dict(), None, FUSED_HEAD + (7, 0x30000000, 832) + mid + (0, 1, None) + rec),
             (dict(ke_out=KE, implicit_drag=True, rotational=False), SO,
              FUSED_HEAD + (7, 0x50000000, 832) + mid + (1, 0, 0x60000000) + rec)]
    for kw, state_out, want in cases:
        lib.calls.clear()
        got = eng.step_fused_tiled_multi_rec(S, P13, N, DT, 7, log, 4, 1, 2, state_out=state_out, stream=STREAM, **kw)
        assert got == 0                                      # the rows the (fake) kernel reported
        assert lib.calls == [("hydro_step_fused_tiled_multi_rec", want)]


def test_fused_refusals(lib, eng):
    tiled = "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0"
    ke = "ke_out: expected a contiguous float64 tensor of 2 elements on cuda:0"
    logmsg = "log must be a contiguous float32 (rows, 13 | 19, columns) tensor on the engine's device"
    log = T((10, 13, 8), 0x80000000)
    for fn, extra in ((eng.step_fused_tiled, ()), (eng.step_fused_tiled_multi, (3,)),
                      (eng.step_fused_tiled_multi_rec, (3, log, 1, 0, 0))):
        refused(lib, tiled, fn, P6, P13, N, DT, *extra, stream=STREAM)
        refused(lib, tiled, fn, S, P6, N, DT, *extra, stream=STREAM)
        refused(lib, tiled, fn, S, P13, N, DT, *extra, state_out=O, stream=STREAM)
        refused(lib, tiled.replace("16", "17"), fn, S, P13, 1025, DT, *extra, stream=STREAM)
        refused(lib, ke, fn, S, P13, N, DT, *extra, stream=STREAM, ke_out=T((2,), 0x1000))
        refused(lib, ke, fn, S, P13, N, DT, *extra, stream=STREAM, ke_out=T((1,), 0x1000, dtype=torch.float64))
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0",
            eng.step_fused_tiled, S, P13, N, DT, wrench=S, stream=STREAM)
    for bad in (T((10, 14, 8), 0x1000), T((10, 13), 0x1000), T((10, 13, 8), 0x1000, dtype=torch.float64),
                T((10, 13, 8), 0x1000, contiguous=False), T((10, 13, 8), 0x1000, device=torch.device("cpu"))):
        refused(lib, logmsg, eng.step_fused_tiled_multi_rec, S, P13, N, DT, 3, bad, 1, 0, 0, stream=STREAM)


# ---------------------------------------------------------------------------------- refusals of a tiled buffer
BAD_STATE = [T((TILES, 12, 64), 0x1000),                                   # wrong field count
             T((TILES - 1, 13, 64), 0x1000),                               # too few tiles
             T((TILES, 13, 64), 0x1000, dtype=torch.float64),              # wrong dtype
             T((TILES, 13, 64), 0x1000, device=torch.device("cuda:1")),    # wrong device
             T((TILES, 13, 64), 0x1000, device=torch.device("cpu")),
             T((TILES, 13, 64), 0x1000, contiguous=False),                 # non-contiguous
             T((TILES, 13, 32), 0x1000),                                   # not a 64-body tile
             T((TILES * 13, 64), 0x1000)]                                  # not 3-D


@pytest.mark.parametrize("prepared", [False, True])
def test_step_wrench_tiled_refusals(lib, eng, prepared):
    fn = eng.prepare_step_wrench_tiled if prepared else eng.step_wrench_tiled
    state = "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0"
    six = "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0"
    for bad in BAD_STATE:
        refused(lib, state, fn, bad, N, DT, out=O, prev=P6, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 17, 13, 64) tensor on cuda:0", fn, S, 1025, DT, out=O, stream=STREAM)
    for bad in (S, T((TILES - 1, 6, 64), 0x1000), T((TILES, 6, 64), 0x1000, dtype=torch.float16),
                T((TILES, 6, 64), 0x1000, device=torch.device("cuda:1")), T((TILES, 6, 64), 0x1000, contiguous=False)):
        refused(lib, six, fn, S, N, DT, out=bad, prev=P6, stream=STREAM)
    # prev: 13 fields are checked as a state buffer, anything else as a 6-field one
    refused(lib, state, fn, S, N, DT, out=O, prev=T((TILES - 1, 13, 64), 0x1000), stream=STREAM)
    refused(lib, state, fn, S, N, DT, out=O, prev=T((TILES, 13, 64), 0x1000, contiguous=False), stream=STREAM)
    refused(lib, six, fn, S, N, DT, out=O, prev=T((TILES, 7, 64), 0x1000), stream=STREAM)
    refused(lib, six, fn, S, N, DT, out=O, prev=T((TILES - 1, 6, 64), 0x1000), stream=STREAM)
    refused(lib, six, fn, S, N, DT, out=O, prev=T((TILES, 6, 64), 0x1000, dtype=torch.float64), stream=STREAM)
    ke = "ke_out: expected a contiguous float64 tensor of 2 elements on cuda:0"
    for bad in (T((2,), 0x1000), T((1,), 0x1000, dtype=torch.float64), T((2,), 0x1000, dtype=torch.float64, contiguous=False),
                T((2,), 0x1000, dtype=torch.float64, device=torch.device("cpu"))):
        refused(lib, ke, fn, S, N, DT, out=O, prev=P6, stream=STREAM, ke_out=bad)


# --------------------------------------------------------------------------- integrator, packing, layout moves
def test_integrate_tiled(lib, eng):
    assert eng.integrate_tiled(S, O, N, DT, state_out=SO, stream=STREAM) is SO
    assert lib.calls == [("hydro_integrate_tiled", (H, 1000, 0x10000000, 832, 0x40000000, 384, 0.01, 0x50000000, 832, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.integrate_tiled, O, O, N, DT, state_out=SO, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.integrate_tiled, S, S, N, DT, state_out=SO, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.integrate_tiled, S, O, N, DT, state_out=O, stream=STREAM)


def test_pack_state_aos(lib, eng):
    for q in (False, True):
        lib.calls.clear()
        assert eng.pack_state_aos(POS, ORI, VELS, out=S, quat_xyzw=q, stream=STREAM) is S
        assert lib.calls == [("hydro_pack_state_aos", (H, 1000, 0x70000000, 0x71000000, int(q), 0x72000000, 0x10000000, 832, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.pack_state_aos, POS, ORI, VELS, out=O, stream=STREAM)


def test_unpack_wrench_aos(lib, eng):
    assert eng.unpack_wrench_aos(O, N, F, TQ, STREAM) == (F, TQ)
    assert lib.calls == [("hydro_unpack_wrench_aos", (H, 1000, 0x40000000, 384, 0x73000000, 0x74000000, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", eng.unpack_wrench_aos, S, N, F, TQ, STREAM)


def test_to_tiled_and_from_tiled(lib, eng):
    soa = T((13, N), 0x90000000)
    tab = tuple(0x90000000 + f * 4000 for f in range(13))
    assert eng.to_tiled(soa, out=S, stream=STREAM) is S
    assert lib.calls == [("hydro_repack", (H, 1000, 13, tab, 0x10000000, 832, 1, STREAM))]
    lib.calls.clear()
    assert eng.from_tiled(S, N, out=soa, stream=STREAM) is soa
    assert lib.calls == [("hydro_repack", (H, 1000, 13, tab, 0x10000000, 832, 0, STREAM))]
    lib.calls.clear()
    w = T((6, 100), 0x91000000)
    eng.from_tiled(O, 100, out=w, stream=STREAM)
    assert lib.calls == [("hydro_repack", (H, 100, 6, tuple(0x91000000 + f * 400 for f in range(6)), 0x40000000, 384, 0, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.to_tiled, soa, out=O, stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 17, 6, 64) tensor on cuda:0", eng.from_tiled, O, 1025, out=w, stream=STREAM)
    refused(lib, "expected contiguous float32 (6,N) tensor on cuda:0", eng.from_tiled, O, 100,
            out=T((6, 100), 0x92000000, dtype=torch.float64), stream=STREAM)


# ---------------------------------------------------------------------------------------------- array of structs
@pytest.mark.parametrize("q", [False, True])
def test_step_wrench_aos(lib, eng, q):
    head, tail = (H, 1000, 0x70000000, 0x71000000, int(q), 0x72000000), (0x73000000, 0x74000000, STREAM)
    assert eng.step_wrench_aos(POS, ORI, VELS, DT, F, TQ, quat_xyzw=q, stream=STREAM) == (F, TQ)
    assert lib.calls == [("hydro_step_wrench_aos", head + (0.01,) + tail)]
    lib.calls.clear()
    step = eng.prepare_step_wrench_aos(POS, ORI, VELS, F, TQ, quat_xyzw=q)
    assert lib.calls == []
    assert step(DT, STREAM) == (F, TQ) and step(DT, stream=STREAM) == (F, TQ) and step(0.02, STREAM) == (F, TQ)

    class Stream:
        cuda_stream = 0x7700
    step(0.02, Stream())
    assert lib.calls == [("hydro_step_wrench_aos", head + (0.01,) + tail), ("hydro_step_wrench_aos", head + (0.01,) + tail),
                         ("hydro_step_wrench_aos", head + (0.02,) + tail),
                         ("hydro_step_wrench_aos", head + (0.02, 0x73000000, 0x74000000, 0x7700))]


def test_step_wrench_aos_refusals(lib, eng):
    row = "expected contiguous float32 (1000,{}) tensor on cuda:0"
    for fn in (lambda p, o, v: eng.step_wrench_aos(p, o, v, DT, F, TQ, stream=STREAM),
               lambda p, o, v: eng.prepare_step_wrench_aos(p, o, v, F, TQ)):
        refused(lib, row.format(3), fn, T((N, 4), 0x1000), ORI, VELS)
        refused(lib, row.format(3), fn, T((N, 3), 0x1000, dtype=torch.float64), ORI, VELS)
        refused(lib, row.format(4), fn, POS, T((N, 3), 0x1000), VELS)
        refused(lib, row.format(4), fn, POS, T((N, 4), 0x1000, contiguous=False), VELS)
        refused(lib, row.format(6), fn, POS, ORI, T((N - 1, 6), 0x1000))
        refused(lib, row.format(6), fn, POS, ORI, T((N, 6), 0x1000, device=torch.device("cpu")))
    # the prepared form also checks the outputs; the direct form passes them on as they are
    out = "expected contiguous float32 (1000,3) output on cuda:0"
    for bad in (T((N, 4), 0x1000), T((N, 3), 0x1000, dtype=torch.float64), T((N, 3), 0x1000, contiguous=False),
                T((N, 3), 0x1000, device=torch.device("cuda:1"))):
        refused(lib, out, eng.prepare_step_wrench_aos, POS, ORI, VELS, bad, TQ)
        refused(lib, out, eng.prepare_step_wrench_aos, POS, ORI, VELS, F, bad)
    odd = T((N, 4), 0x76000000, dtype=torch.float64)
    assert eng.step_wrench_aos(POS, ORI, VELS, DT, odd, TQ, stream=STREAM) == (odd, TQ)
    assert lib.calls == [("hydro_step_wrench_aos", (H, 1000, 0x70000000, 0x71000000, 0, 0x72000000, 0.01, 0x76000000, 0x74000000, STREAM))]


# ---------------------------------------------------------------------- component mode, energy, plain SoA wrench
def test_step_components(lib, eng):
    state, accel, out = T((13, N), 0x90000000), T((6, N), 0x91000000), T((24, N), 0x92000000)
    assert eng.step_components(state, accel, out=out, ratio=RATIO, stream=STREAM) == (out, RATIO)
    assert lib.calls == [("hydro_step_components", (H, 1000, tuple(0x90000000 + 4000 * f for f in range(13)),
                                                    tuple(0x91000000 + 4000 * f for f in range(6)),
                                                    tuple(0x92000000 + 4000 * f for f in range(24)), 0x75000000, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (6,N) tensor on cuda:0", eng.step_components, state, T((5, N), 0x93000000),
            out=out, ratio=RATIO, stream=STREAM)


def test_step_components_aos(lib, eng):
    ins = [T((N, w), 0xA0000000 + 0x100000 * i) for i, w in enumerate((3, 4, 3, 3, 3, 3))]
    ptrs = (0xA0000000, 0xA0100000, 0xA0200000, 0xA0300000, 0xA0400000, 0xA0500000)
    out = T((8, N, 3), 0xB0000000)
    tab = tuple(0xB0000000 + k * 12000 for k in range(8))
    assert eng.step_components_aos(*ins, out, ratio=RATIO, stream=STREAM) is out
    assert eng.step_components_aos(*ins, out, stream=STREAM) is out
    assert lib.calls == [("hydro_step_components_aos", (H, 1000) + ptrs + (tab, 0x75000000, STREAM)),
                         ("hydro_step_components_aos", (H, 1000) + ptrs + (tab, None, STREAM))]
    lib.calls.clear()
    row = "expected contiguous float32 (1000,{}) tensor on cuda:0"
    for i, w in enumerate((3, 4, 3, 3, 3, 3)):
        bad = list(ins)
        bad[i] = T((N, w + 1), 0x1000)
        refused(lib, row.format(w), eng.step_components_aos, *bad, out, stream=STREAM)
    for bad in (T((8, N, 4), 0x1000), T((7, N, 3), 0x1000), T((8, N, 3), 0x1000, dtype=torch.float64),
                T((8, N, 3), 0x1000, contiguous=False), T((8, N, 3), 0x1000, device=torch.device("cpu"))):
        refused(lib, "expected contiguous float32 (8,1000,3) output on cuda:0", eng.step_components_aos, *ins, bad, stream=STREAM)


def test_kinetic_energy(lib, eng):
    soa = T((13, 500), 0x90000000)
    for rot in (False, True):
        lib.calls.clear()
        assert eng.kinetic_energy(S, rotational=rot, out=KE, stream=STREAM) is KE
        assert eng.kinetic_energy(soa, rotational=rot, out=KE, stream=STREAM) is KE
        assert lib.calls == [("hydro_kinetic_energy_tiled", (H, 1000, 0x10000000, 832, int(rot), 0x60000000, STREAM)),
                             ("hydro_kinetic_energy", (H, 500, tuple(0x90000000 + 2000 * f for f in range(13)), int(rot),
                                                       0x60000000, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", eng.kinetic_energy, O, out=KE, stream=STREAM)


def test_step_wrench(lib, eng):
    state, prev, out = T((13, N), 0x90000000), T((6, N), 0x91000000), T((6, N), 0x92000000)
    ts, tp, to = table(state), table(prev), table(out)
    assert ts[1] - ts[0] == 4000 and len(ts) == 13 and len(tp) == 6
    assert eng.step_wrench(state, DT, out=out, stream=STREAM) is out
    assert eng.step_wrench(state, DT, out=out, prev=prev, stream=STREAM) is out
    assert lib.calls == [("hydro_step_wrench", (H, 1000, ts, 0.01, to, STREAM)),
                         ("hydro_step_wrench_ext", (H, 1000, ts, tp, 0.01, to, STREAM))]
    lib.calls.clear()
    refused(lib, "expected contiguous float32 (13,N) tensor on cuda:0", eng.step_wrench, T((12, N), 0x93000000), DT,
            out=out, stream=STREAM)
