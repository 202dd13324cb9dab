"""The applied wrench (hydro_step_fused_tiled_multi_app, HydroEngine.step_fused_tiled_multi_applied) as far as a machine
without a GPU can see it: the C boundary, the null-handle refusals, the Python host's marshalling (with the stand-ins of
tests/test_engine_calls.py) and the generated code - the new kernel's instantiations exist, none spills, and the plain
resident loop is the code profiles/isa_mix.json records."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO
from silver2_isaacsim_amd import _native as nat
from silver2_isaacsim_amd import build as hb
from engine_stand_ins import DEV, eng, FUSED_HEAD, KE, lib, N, P13, refused, S, SO, STREAM, T, TILES  # noqa: F401  (fixtures are requested by name)

ENTRY = "hydro_step_fused_tiled_multi_app"
A = T((TILES, 6, 64), 0x88000000)                                # the applied wrench's stand-in


# ---- C boundary ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry():
    text = open(os.path.join(REPO, "include", "hydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + ENTRY + r"\s*\(", code) and ENTRY in nat.SIGNATURES
    assert "#define HYDRO_VERSION 0x000701" in text              # an addition to 0.7.1, not a new version
    assert int(re.search(r"#define HYDRO_FRAME_WORLD\s+(\d+)", code).group(1)) == nat.HYDRO_FRAME_WORLD == 0
    assert int(re.search(r"#define HYDRO_FRAME_BODY\s+(\d+)", code).group(1)) == nat.HYDRO_FRAME_BODY == 1
    # the recording entry's argument list with (applied, applied_tile_stride, applied_frame) in front of the stream
    rec, app = nat.SIGNATURES["hydro_step_fused_tiled_multi_rec"], nat.SIGNATURES[ENTRY]
    assert app[0] is rec[0]
    assert app[1] == rec[1][:-1] + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + rec[1][-1:]
    # and so says the header: the text between the parentheses of the two prototypes
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1))  # noqa: E731
    assert proto(ENTRY) == proto("hydro_step_fused_tiled_multi_rec").replace(
        ", void *stream", ", const float *applied, int64_t applied_tile_stride, int applied_frame, void *stream")


@pytest.mark.parametrize("applied,log", [(None, None), (0x1000, None), (None, 0x2000), (0x1000, 0x2000), (0x1001, 0x2000)])
@pytest.mark.parametrize("stride,frame", [(384, 0), (384, 1), (383, 0), (384, 2)])
def test_null_handle_gives_e_arg_without_a_device(native_built, applied, log, stride, frame):
    lib = nat.load()
    written = ctypes.c_int64(-7)
    rc = getattr(lib, ENTRY)(None, 64, None, 832, None, 832, 1 / 60, 4, None, 832, None, 832, 0, 0, None,
                             log, 1, 4, 13, 1, 1, 0, ctypes.byref(written), applied, stride, frame, None)
    assert rc == -1 and written.value == -7                      # nothing written, not even the row count


# ---- marshalling ------------------------------------------------------------------------------------------------------------
NO_LOG = (None, 0, 0, 13, 1, 1, 0, ("byref", 0))


@pytest.mark.parametrize("frame,code", [("world", 0), ("body", 1)])
def test_step_fused_tiled_multi_applied(lib, eng, frame, code):
    mid = (0x10000000 + 1792, 832)
    app = (0x88000000, 384, code, STREAM)
    log = T((10, 19, 8), 0x80000000)
    rec = (0x80000000, 8, 10, 19, 4, 2, 3, ("byref", 0))
    cases = [(dict(), None, FUSED_HEAD + (7, 0x30000000, 832) + mid + (0, 1, None) + NO_LOG + app),
             (dict(ke_out=KE, implicit_drag=True, rotational=False), SO,
              FUSED_HEAD + (7, 0x50000000, 832) + mid + (1, 0, 0x60000000) + NO_LOG + app),
             (dict(log=log, every=4, phase=2, row0=3), None, FUSED_HEAD + (7, 0x30000000, 832) + mid + (0, 1, None) + rec + app)]
    for kw, state_out, want in cases:
        lib.calls.clear()
        got = eng.step_fused_tiled_multi_applied(S, P13, N, 0.01, 7, A, frame, state_out=state_out, stream=STREAM, **kw)
        assert got == 0                                          # the rows the (fake) kernel reported
        assert lib.calls == [(ENTRY, want)]


def test_defaults_and_no_wrench(lib, eng):
    """frame defaults to the body frame; applied=None goes to the same entry with a null pointer (the library then runs the
    unapplied kernels); steps = 1 is the single-step form."""
    eng.step_fused_tiled_multi_applied(S, P13, N, 0.01, 1, A, stream=STREAM)
    eng.step_fused_tiled_multi_applied(S, P13, N, 0.01, 1, None, "world", stream=STREAM)
    head = FUSED_HEAD + (1, 0x30000000, 832, 0x10000000 + 1792, 832, 0, 1, None) + NO_LOG
    assert lib.calls == [(ENTRY, head + (0x88000000, 384, 1, STREAM)), (ENTRY, head + (None, 0, 0, STREAM))]


def test_applied_refusals(lib, eng):
    six = "expected contiguous float32 (>= 16, 6, 64) tensor on cuda:0"
    fn = eng.step_fused_tiled_multi_applied
    for bad in (T((TILES, 6, 64), 0x1000, dtype=torch.float64), T((TILES, 6, 64), 0x1000, dtype=torch.float16),
                T((TILES, 6, 64), 0x1000, device=torch.device("cpu")), T((TILES, 6, 64), 0x1000, device=torch.device("cuda:1")),
                T((TILES, 7, 64), 0x1000), T((TILES - 1, 6, 64), 0x1000), T((TILES * 64, 6), 0x1000), S,
                T((TILES, 6, 64), 0x1000, contiguous=False)):
        refused(lib, six, fn, S, P13, N, 0.01, 3, bad, "world", stream=STREAM)
    for bad in ("Body", "local", 1, None):
        refused(lib, "frame must be 'world' or 'body'", fn, S, P13, N, 0.01, 3, A, bad, stream=STREAM)
    # what the neighbours refuse
    refused(lib, "expected contiguous float32 (>= 16, 13, 64) tensor on cuda:0", fn, A, P13, N, 0.01, 3, A, stream=STREAM)
    refused(lib, "log must be a contiguous float32 (rows, 13 | 19, columns) tensor on the engine's device",
            fn, S, P13, N, 0.01, 3, A, log=T((10, 14, 8), 0x1000), stream=STREAM)
    refused(lib, "ke_out: expected a contiguous float64 tensor of 2 elements on cuda:0", fn, S, P13, N, 0.01, 3, A,
            ke_out=T((2,), 0x1000), stream=STREAM)


# ---- generated code ------------------------------------------------------------------------------------------------------------
APP = "step_fused_multi_app_tiled_kernel"
PLAIN_LOOP = "step_fused_multi_tiled_kernelILb0ELb0ELb0ELb0ELb0E"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "hydro.s")
    cmd = [hb.hipcc_path()] + hb.device_flags() + ["--cuda-device-only", "-S", "-o", out, hb.SRC]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(out))
    assert res.returncode == 0, res.stderr[-3000:]
    return open(out).read()


def test_applied_kernel_code(assembly):
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", assembly, re.S)}
    app = {k: d for k, d in desc.items() if APP in k}
    flags = {re.search(r"kernelI((?:Lb\dE){5})", k).group(1) for k in app}               # <HALF, NT, IMPLICIT, KE, WARP>
    assert len(app) == len(flags) == 32                          # one per flag combination: it serves "applied" and "applied + recorder"
    for name, d in app.items():
        assert int(d["private_segment_fixed_size"]) == 0, name   # no spill
        assert int(d["next_free_vgpr"]) <= 168, (name, d["next_free_vgpr"])              # 3 waves per SIMD, like the resident kernels
    print("[applied kernel] VGPRs %d .. %d, SGPRs %d .. %d over the 32 instantiations" % (
        min(int(d["next_free_vgpr"]) for d in app.values()), max(int(d["next_free_vgpr"]) for d in app.values()),
        min(int(d["next_free_sgpr"]) for d in app.values()), max(int(d["next_free_sgpr"]) for d in app.values())))


def test_plain_resident_loop_is_the_recorded_code(assembly):
    """The no-op policy compiles to nothing: the body of the plain resident kernel has the VALU count profiles/isa_mix.json
    records for it."""
    committed = json.load(open(os.path.join(REPO, "profiles", "isa_mix.json")))["kernels"]
    want = next(v for k, v in committed.items() if k.startswith("resident closed loop, one step (step_fused_multi_tiled_kernel<f32 parameters"))
    body = re.search(r"^(_Z\S*" + PLAIN_LOOP + r"[^\s:]*):[^\n]*\n(.*?)s_endpgm", assembly, re.S | re.M).group(2)
    loop = re.search(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)^\s+s_branch \1$", body, re.S | re.M).group(2)
    valu = [op for op in re.findall(r"^\s+([a-z][a-z0-9_]+)", loop, re.M) if op.startswith("v_")]
    assert len(valu) == want["valu_total"]
