"""The pose hold (hydro_step_fused_tiled_multi_ctl, HydroEngine.step_fused_tiled_multi_controlled) as far as a machine
without a GPU can see it: the C boundary, the null-handle refusal, the Python host's marshalling (with the stand-ins of
tests/test_engine_calls.py), and the fp64 restatement of the law (tests/pose_hold_reference.py) on literal cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pose_hold_reference as phr
from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from engine_stand_ins import DEV, eng, FUSED_HEAD, KE, lib, N, P13, refused, S, SO, STREAM, T, TILES  # noqa: F401  (fixtures are requested by name)

ENTRY = "hydro_step_fused_tiled_multi_ctl"
A = T((TILES, 6, 64), 0x88000000)                                # the applied wrench's stand-in
C = T((TILES, 17, 64), 0x90000000)                               # the control record's


# ---- C boundary ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + ENTRY + r"\s*\(", code) and ENTRY in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert int(re.search(r"#define HYDRO_CTL_FIELDS\s+(\d+)", code).group(1)) == nat.CTL_FIELDS == phr.FIELDS == 17
    # the applied entry's argument list with (control, control_tile_stride) in front of the stream
    app, ctl = nat.SIGNATURES["hydro_step_fused_tiled_multi_app"], nat.SIGNATURES[ENTRY]
    assert ctl[0] is app[0]
    assert ctl[1] == app[1][:-1] + [ctypes.c_void_p, ctypes.c_int64] + app[1][-1:]
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_app").replace(
        ", void *stream", ", const float *control, int64_t control_tile_stride, void *stream")


def test_library_exports_the_entry(native_built):
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + ENTRY + r"$", out, re.M)
    assert hasattr(nat.load(), ENTRY)


@pytest.mark.parametrize("applied,control,stride", [(None, None, 0), (None, 0x1000, 1088), (0x2000, 0x1000, 1088), (None, 0x1004, 1088),
                                                    (None, 0x1000, 1087)])
def test_null_handle_gives_e_arg_without_a_device(native_built, applied, control, stride):
    written = ctypes.c_int64(-7)
    rc = getattr(nat.load(), ENTRY)(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                                    None, 1, 4, 13, 1, 1, 0, ctypes.byref(written), applied, 384, 0, control, stride, None)
    assert rc == nat.HYDRO_E_ARG == -1 and written.value == -7   # nothing written, not even the row count


# ---- marshalling ------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))
MID = (0x10000000 + 1792, 832)


def test_step_fused_tiled_multi_controlled(lib, eng):
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    ctl = (0x90000000, 1088, STREAM)
    cases = [(dict(), None, FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG + (None, 0, 1) + ctl),
             (dict(applied=A, frame="world", ke_out=KE, implicit_drag=True, rotational=False), SO,
              FUSED_HEAD + (7, 0x50000000, 832) + MID + (1, 0, 0x60000000) + NO_LOG + (0x88000000, 384, 0) + ctl),
             (dict(applied=A, log=log, every=4, phase=2, row0=3), None,
              FUSED_HEAD + (7, 0x30000000, 832) + MID + (0, 1, None) + rec + (0x88000000, 384, 1) + ctl)]
    for kw, state_out, want in cases:
        lib.calls.clear()
        assert eng.step_fused_tiled_multi_controlled(S, P13, N, 0.01, 7, C, state_out=state_out, stream=STREAM, **kw) == 0
        assert lib.calls == [(ENTRY, want)]


def test_no_control_goes_to_the_same_entry_with_a_null_pointer(lib, eng):
    """(the library then launches what the applied entry launches)"""
    eng.step_fused_tiled_multi_controlled(S, P13, N, 0.01, 1, None, A, "world", stream=STREAM)
    head = FUSED_HEAD + (1, 0x30000000, 832) + MID + (0, 1, None) + NO_LOG
    assert lib.calls == [(ENTRY, head + (0x88000000, 384, 0, None, 0, STREAM))]


def test_controlled_refusals(lib, eng):
    want = "expected contiguous float32 (>= 16, 17, 64) tensor on cuda:0"
    fn = eng.step_fused_tiled_multi_controlled
    for bad in (T((TILES, 17, 64), 0x1000, dtype=torch.float64), T((TILES, 17, 64), 0x1000, device=torch.device("cpu")),
                T((TILES, 16, 64), 0x1000), T((TILES - 1, 17, 64), 0x1000), T((TILES * 64, 17), 0x1000), A, S,
                T((TILES, 17, 64), 0x1000, contiguous=False)):
        refused(lib, want, fn, S, P13, N, 0.01, 3, bad, stream=STREAM)
    refused(lib, "frame must be 'world' or 'body'", fn, S, P13, N, 0.01, 3, C, A, "local", stream=STREAM)
    refused(lib, "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0", fn, S, P13, N, 0.01, 3, C, C, stream=STREAM)


# ---- the law, by hand ----------------------------------------------------------------------------------------------------------
def _body(p=(0.0, 0.0, 0.0), q=(0.0, 0.0, 0.0, 1.0), v=(0.0, 0.0, 0.0), w=(0.0, 0.0, 0.0)):
    return np.array([[*p, *q, *v, *w]], np.float64)


def test_a_displaced_body_is_pulled_back_along_the_displacement():
    s = _body(p=(1.5, -2.0, 0.25))
    c = phr.record(1, position=(1.0, -2.0, 0.25), orientation_xyzw=(0, 0, 0, 1), kp_lin=8.0)
    assert np.array_equal(phr.wrench(s, c), [[-4.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    # per-axis gains: a pure depth hold ignores the horizontal error; the damping opposes the velocity
    s = _body(p=(3.0, 4.0, -1.0), v=(0.5, 0.0, 2.0))
    c = phr.record(1, position=(0.0, 0.0, -3.0), orientation_xyzw=(0, 0, 0, 1), kp_lin=(0.0, 0.0, 10.0), kd_lin=(0.0, 0.0, 4.0))
    assert np.array_equal(phr.wrench(s, c), [[0.0, 0.0, -20.0 - 8.0, 0.0, 0.0, 0.0]])


def test_a_yaw_error_of_plus_30_degrees_gives_a_minus_z_torque():
    half = np.radians(15.0)
    s = _body(q=(0.0, 0.0, np.sin(half), np.cos(half)), w=(0.0, 0.0, 0.5))
    c = phr.record(1, position=0.0, orientation_xyzw=(0, 0, 0, 1), kp_ang=3.0, kd_ang=0.25)
    want = -3.0 * 2.0 * np.sin(half) - 0.25 * 0.5
    got = phr.wrench(s, c.astype(np.float64))
    assert np.allclose(got, [[0, 0, 0, 0, 0, want]], rtol=0, atol=1e-15) and got[0, 5] < 0
    # the same attitude written as -q is the same rotation: the same torque (the sign flip)
    assert np.allclose(phr.wrench(_body(q=(0.0, 0.0, -np.sin(half), -np.cos(half)), w=(0.0, 0.0, 0.5)), c), got, rtol=0, atol=1e-15)
    assert phr.error_quaternion(_body(q=(0.0, 0.0, -np.sin(half), -np.cos(half))), c)[0, 3] < 0
    # the rotation vector to first order: for a small angle a about a unit axis, e_r = a * axis
    a, axis = 1e-4, np.array([2.0, -1.0, 2.0]) / 3.0
    tgt = (*(np.sin(a / 2) * axis), np.cos(a / 2))
    c = phr.record(1, position=0.0, orientation_xyzw=0.0, kp_ang=1.0).astype(np.float64)
    c[0, 3:7] = tgt
    assert np.allclose(phr.wrench(_body(), c)[0, 3:6], a * axis, rtol=1e-8, atol=0)


def test_the_clamp_caps_the_norm_and_keeps_the_direction():
    s = _body(p=(3.0, 4.0, 12.0))
    c = phr.record(1, position=0.0, orientation_xyzw=(0, 0, 0, 1), kp_lin=2.0, f_max=6.5)
    got = phr.wrench(s, c)[0, 0:3]                               # unclamped: -(6, 8, 24), norm 26
    assert np.isclose(np.linalg.norm(got), 6.5, rtol=1e-15) and np.allclose(got, -np.array([3.0, 4.0, 12.0]) / 13.0 * 6.5, rtol=1e-15)
    assert phr.saturated(s, c)[0].all() and not phr.saturated(s, c)[1].any()
    # below the limit nothing changes, at the limit the clamp is continuous, f_max = 0 switches the force off
    for top, want in ((26.0, (-6.0, -8.0, -24.0)), (np.inf, (-6.0, -8.0, -24.0)), (0.0, (0.0, 0.0, 0.0))):
        c[0, phr.F_MAX] = top
        assert np.allclose(phr.wrench(s, c)[0, 0:3], want, rtol=1e-15, atol=0)
    # the torque clamp likewise
    s = _body(w=(0.0, 3.0, 4.0))
    c = phr.record(1, position=0.0, orientation_xyzw=(0, 0, 0, 1), kd_ang=2.0, t_max=1.0)
    assert np.allclose(phr.wrench(s, c)[0, 3:6], (0.0, -0.6, -0.8), rtol=1e-15)
