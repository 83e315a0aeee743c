"""bf16 training maps (include/csn_hip.h section 28, csn_amd/csrc/train_maps16.hip, ``tuning.train_maps16``), checked without a GPU:
the switch; the exports against the header and the binding; every host-side argument check of the four entry points with made-up
pointers (nothing is launched); the Python route's refusals — a CPU tensor, the wrong mode, an fp16 tensor; and the registers, LDS
and waves per SIMD of the thirteen new kernel instances, read from a compile for gfx950 (the figures of DESIGN.md "16-bit
training maps")."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import sparse_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["csn_sparse_conv_stats_fwd_t16", "csn_rows_bn_act_fwd_t16", "csn_rows_bn_act_bwd_t16", "csn_sparse_conv_bwd_t16"]
ARG, ALIGN, PTR, DIM, WORKSPACE = -1, -2, -3, -5, -6
FAKE, OTHER = 1 << 20, 1 << 22


@pytest.fixture()
def lib16():
    """The library in math mode 2 with the rows16 flag set; both restored afterwards."""
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    L.csn_set_thread_math_mode(2)
    L.csn_set_thread_rows16(1)
    yield L
    L.csn_set_thread_rows16(0)
    L.csn_set_thread_math_mode(-1)


def test_the_switch_defaults_to_off_and_round_trips():
    from csn_amd import tuning
    assert tuning.Tuning().train_maps16 is False and tuning.current().train_maps16 is False
    with tuning.override(train_maps16=True) as t:
        assert t.train_maps16 is True and tuning.current().train_maps16 is True
        with tuning.override(train_maps16=False):
            assert tuning.current().train_maps16 is False
    assert tuning.current().train_maps16 is False


def test_the_exports_agree_with_the_header_and_the_binding():
    import csn_amd
    from csn_amd import _lib
    _lib.build()
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as fh:
        header = fh.read()
    kinds = {"*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float}
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        m = re.search(r"CSN_API int " + name + r"\(([^;]*)\);", header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [kinds["*"] if "*" in p else kinds[" ".join(p.split()[:-1]).replace("const ", "")] for p in params]
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and args == want, name
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert "(28)" in header and header.index("(28)") > header.index("(27)")
    assert "train_maps16.hip" in _lib.SOURCES and _lib.lib().csn_version() == 17
    for name in ("Map16", "train_maps16_open", "conv_stats", "bn_act"):
        assert hasattr(csn_amd, name), name


def _stats(L, x=FAKE, x16=1, ld_x=64, n_in=13, table=FAKE, n_out=11, kv=27, c_in=64, c_out=32, w=FAKE, z=FAKE, ld_z=32, mean=FAKE,
           invstd=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return L.csn_sparse_conv_stats_fwd_t16(x, x16, ld_x, n_in, table, n_out, kv, c_in, c_out, w, z, ld_z, mean, invstd, None, None, 1e-5, 0.1,
                                           ws, ws_bytes, None)


def _wgrad(L, dy=FAKE, ld_dy=32, x=FAKE, x16=1, ld_x=64, n_in=13, n_out=11, kv=27, c_in=64, c_out=32, fwd=FAKE, w=FAKE, dx=None, dw=OTHER,
           ws=FAKE, ws_bytes=1 << 30):
    return L.csn_sparse_conv_bwd_t16(dy, ld_dy, x, x16, ld_x, n_in, n_out, kv, c_in, c_out, fwd, None, w, dx, 64, dw, None, ws, ws_bytes, None)


def _terms(_lib, z=FAKE, ld_z=32):
    t = _lib.BnTerms()
    t.z[0], t.ld_z[0], t.mean[0], t.scale[0], t.gamma[0], t.beta[0] = z, ld_z, FAKE, FAKE, FAKE, FAKE
    return t


def _fwd(L, t, n=9, C=32, r=OTHER, r16=1, ld_r=32, y=FAKE, y16=1, ld_y=32):
    return L.csn_rows_bn_act_fwd_t16(ctypes.addressof(t), 1, n, C, 1, 1e-5, r, r16, ld_r, 1, y, y16, ld_y, None)


def _bwd(L, t, n=9, C=32, dy=FAKE, y=FAKE, y16=1, ld_y=32, relu=1, ws=FAKE, ws_bytes=1 << 30):
    return L.csn_rows_bn_act_bwd_t16(dy, 32, y, y16, ld_y, ctypes.addressof(t), 1, n, C, 1, 1e-5, relu, None, 0, ws, ws_bytes, None)


def test_section_28_rejects_bad_arguments_on_the_host(lib16):
    # (every call below fails a check: nothing is ever launched on these made-up addresses)
    from csn_amd import _lib
    L = lib16
    # the convolution: a call valid but for a misaligned x gets past every other check
    assert _stats(L, x=FAKE + 8) == PTR and _stats(L, x16=0, ld_x=64, x=FAKE + 4) == PTR
    for name in ("x", "table", "w", "z", "mean", "invstd", "ws"):
        assert _stats(L, **{name: None}) == ARG, name
    assert _stats(L, x16=2) == ARG and _stats(L, x16=-1) == ARG
    assert _stats(L, ld_x=68) == ALIGN and _stats(L, ld_x=56) == ARG and _stats(L, ld_x=(1 << 20) + 8) == DIM
    assert _stats(L, x16=0, ld_x=68, x=FAKE + 4) == PTR                      # % 4 is the fp32 rule
    n = 1 << 21                                                             # rows * pitch * 2 inside the window, * 4 outside
    assert _stats(L, n_in=n, c_in=256, ld_x=480, x=FAKE + 8) == PTR and _stats(L, n_in=n, c_in=256, ld_x=480, x16=0) == DIM
    assert _stats(L, c_in=40, ld_x=40) == DIM and _stats(L, c_out=288, ld_z=288) == DIM and _stats(L, kv=8) == DIM
    assert _stats(L, ld_z=34) == ALIGN and _stats(L, n_out=1) == ARG and _stats(L, ws_bytes=16) == WORKSPACE
    # the weight gradient
    assert _wgrad(L, x=FAKE + 8) == PTR and _wgrad(L, dw=OTHER + 8) == PTR
    assert _wgrad(L, x16=3) == ARG and _wgrad(L, x=None) == ARG and _wgrad(L, fwd=None) == ARG and _wgrad(L, dy=None) == ARG
    assert _wgrad(L, ld_x=68) == ALIGN and _wgrad(L, ld_x=56) == ARG and _wgrad(L, c_in=48, ld_x=48) == DIM
    assert _wgrad(L, ws_bytes=0, x=FAKE) == WORKSPACE
    # the BatchNorm row kernels
    t = _terms(_lib)
    assert _fwd(L, t, y=FAKE + 8) == PTR and _fwd(L, t, r=OTHER + 8) == PTR
    assert _fwd(L, t, y16=2) == ARG and _fwd(L, t, r16=-1) == ARG and _fwd(L, t, y=None) == ARG
    assert _fwd(L, t, ld_y=36) == ALIGN and _fwd(L, t, ld_r=36) == ALIGN and _fwd(L, t, ld_y=24) == ARG
    assert _fwd(L, t, y16=0, ld_y=36, y=FAKE + 8) == PTR and _fwd(L, t, r=None, ld_r=3, y=FAKE + 8) == PTR
    assert _fwd(L, t, C=40) == DIM and _fwd(L, t, n=0) == ARG and _fwd(L, _terms(_lib, z=FAKE + 8)) == PTR
    assert _bwd(L, t, y=FAKE + 8) == PTR and _bwd(L, t, y16=2) == ARG and _bwd(L, t, y=None) == ARG and _bwd(L, t, dy=None) == ARG
    assert _bwd(L, t, ld_y=36) == ALIGN and _bwd(L, t, ld_y=24) == ARG and _bwd(L, t, ws_bytes=16) == WORKSPACE
    assert _bwd(L, t, y16=0, ld_y=36, y=FAKE + 4) == PTR


def test_section_28_needs_math_mode_2_with_rows16():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    t = _terms(_lib)
    try:
        for mode, rows16, want in ((0, 1, ARG), (1, 1, ARG), (2, 0, ARG), (3, 1, ARG), (3, 0, ARG), (2, 1, PTR)):
            L.csn_set_thread_math_mode(mode)
            L.csn_set_thread_rows16(rows16)
            # valid but for a misaligned pointer: PTR where the mode admits the call, ARG before any other check where it does not
            assert _stats(L, x=FAKE + 8) == want and _stats(L, x16=0, x=FAKE + 4) == want, (mode, rows16)
            assert _wgrad(L, x=FAKE + 8) == want and _fwd(L, t, y=FAKE + 8) == want and _bwd(L, t, y=FAKE + 8) == want, (mode, rows16)
    finally:
        L.csn_set_thread_rows16(0)
        L.csn_set_thread_math_mode(-1)


def test_python_route_refuses_cpu_tensors_the_wrong_mode_and_fp16():
    from csn_amd import CsnError, Map16, bn_act, bn_act_groups, build_pyramid, conv_stats, conv_stats_groups, train_maps16_open, tuning
    from csn_amd import functional as CF
    kmap = build_pyramid(torch.tensor(R.dense_block()), 2).s1[0]
    w, v = torch.zeros(27, 32, 32), torch.zeros(32)
    edge = torch.zeros(1).expand(64, 32)
    m = Map16(torch.zeros(64, 32, dtype=torch.bfloat16), edge)
    term = (torch.zeros(64, 32), v, v, v, v)
    assert m.shape == (64, 32) and m.detach().dtype == torch.bfloat16 and edge.untyped_storage().nbytes() == 4
    with pytest.raises(ValueError, match="bfloat16, not torch.float16"):
        Map16(torch.zeros(64, 32, dtype=torch.float16), edge)
    with pytest.raises(ValueError, match="same shape"):
        Map16(torch.zeros(64, 32, dtype=torch.bfloat16), torch.zeros(1).expand(64, 64))
    # without the mode, or without rows_single_product: ValueError before anything else
    assert not train_maps16_open()
    for mode, single in (("bf16", False), ("fp16", True), ("fp32", True), ("bf16x3", True)):
        with CF.math_mode(mode), tuning.override(rows_single_product=single):
            assert not train_maps16_open()
            with pytest.raises(ValueError, match="rows_single_product"):
                conv_stats(m, w, kmap, None, None, 1e-5, 0.02)
            with pytest.raises(ValueError, match="rows_single_product"):
                bn_act([term], residual=m)
            with pytest.raises(ValueError, match="rows_single_product"):
                bn_act([term], out_dtype=torch.bfloat16)
    with CF.math_mode("bf16"), tuning.override(rows_single_product=True):
        assert train_maps16_open()
        with pytest.raises(ValueError, match="fp16"):
            bn_act([term], out_dtype=torch.float16)
        # the route is open: CPU tensors are what is left
        with pytest.raises(CsnError, match="no CPU path"):
            conv_stats(m, w, kmap, None, None, 1e-5, 0.02)
        with pytest.raises(CsnError, match="no CPU path"):
            bn_act([term], residual=m)
        with pytest.raises(CsnError, match="no CPU path"):
            bn_act([term], out_dtype=torch.bfloat16)
        # row groups have no bf16-map form
        g = torch.tensor([0, 32, 64], dtype=torch.int32)
        with pytest.raises(ValueError, match="row groups"):
            conv_stats_groups(m, w, kmap, g, None, None, 1e-5, 0.02)
        with pytest.raises(ValueError, match="row groups"):
            bn_act_groups([term], g, residual=m)
    # a plain call is section 15 as ever
    with pytest.raises(CsnError, match="no CPU path"):
        bn_act([term])


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


# kernel -> instance -> (vector registers, accumulator registers, scalar registers, LDS bytes: each at most; waves per SIMD: at
# least): what the compiler reports for gfx950 (DESIGN.md "16-bit training maps")
PINS = {
    "sconv_stats_x16_kernel": {"1": (46, 16, 52, 3572, 8), "2": (66, 32, 84, 6132, 4), "3": (76, 48, 84, 8692, 4), "4": (82, 64, 84, 11252, 3)},
    "sconv_wgrad_x16_kernel": {"1": (106, 16, 45, 8192, 4), "2": (136, 64, 46, 16384, 2), "3": (198, 96, 48, 24576, 1),
                               "4": (246, 144, 46, 32768, 1)},
    "rows_bn_act_fwd16_kernel": {"01": (72, 0, 42, 0, 7), "10": (72, 0, 42, 0, 7), "11": (72, 0, 42, 0, 7)},
    "rows_bn_act_bwd16_kernel": {"1": (110, 0, 54, 32768, 4), "2": (83, 0, 78, 0, 5)},
}


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_train_maps16_instances_keep_registers_lds_and_occupancy(tmp_path):
    """Thirteen instances in the new translation unit and nothing else; no scratch, no spilled registers; vector, accumulator and
    scalar registers, LDS and waves per SIMD as recorded."""
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                               os.path.join(ROOT, "csn_amd", "csrc", "train_maps16.hip"), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {k: {} for k in PINS}
    blocks = re.split(r"Function Name: ", res.stderr)[1:]
    for b in blocks:
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+_kernel)I((?:L[ib]\d+E)+)E", b)
        assert m, b[:120]
        name, inst = m.group(1), "".join(re.findall(r"L[ib](\d+)E", m.group(2)))
        assert name in PINS and inst in PINS[name], (name, inst)
        vgpr, agpr, sgpr, lds, waves = PINS[name][inst]
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, (name, inst)
        got = (field("VGPRs"), field("AGPRs"), field("SGPRs"))
        assert got[0] <= vgpr and got[1] <= agpr and got[2] <= sgpr, (name, inst, got)
        assert field("LDS Size [bytes/block]") <= lds, (name, inst, field("LDS Size [bytes/block]"))
        assert field("Occupancy [waves/SIMD]") >= waves, (name, inst, field("Occupancy [waves/SIMD]"))
        seen[name][inst] = True
    assert {k: sorted(v) for k, v in seen.items()} == {k: sorted(v) for k, v in PINS.items()} and len(blocks) == 13
