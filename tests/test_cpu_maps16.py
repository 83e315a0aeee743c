"""16-bit inference maps (include/csn_hip.h section 24, csn_amd/csrc/sparse_conv_maps16.hip, ``tuning.infer_maps16``), checked without
a GPU: every host-side argument check of ``csn_sparse_conv_bn_act_fwd_m16`` with made-up pointers (nothing is launched); the switch
and the Python route's refusals; the rounding yardstick of tests/test_gpu_maps16.py; and the resources of the sixteen new kernel
instances against the ``sconv_gemm16_bn_kernel`` instance of the same column blocks and mode, read from the same compile."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import rows16_ref as R16
from tests import sparse_conv_ref as R

NAME = "csn_sparse_conv_bn_act_fwd_m16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN, PTR, DIM = -1, -2, -3, -5
FAKE, OTHER = 1 << 20, 1 << 22


@pytest.fixture()
def lib16():
    """The library in math mode 2 with the rows16 flag set; both restored afterwards."""
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    before = L.csn_get_math_mode()
    L.csn_set_thread_math_mode(2)
    L.csn_set_thread_rows16(1)
    yield L
    L.csn_set_thread_rows16(0)
    L.csn_set_thread_math_mode(-1)
    assert L.csn_get_math_mode() == before


def _f(L, x=FAKE, x16=1, ld_x=64, n_in=13, table=FAKE, n_out=11, kv=27, c_in=64, c_out=32, w=FAKE, gamma=FAKE, beta=FAKE, rm=FAKE,
       rv=FAKE, r=OTHER, r16=1, ld_r=32, relu=1, y=FAKE, y16=1, ld_y=32):
    # (every call below fails a check: nothing is ever launched on these made-up addresses)
    return L.csn_sparse_conv_bn_act_fwd_m16(x, x16, ld_x, n_in, table, n_out, kv, c_in, c_out, w, gamma, beta, rm, rv, 1e-5, r, r16, ld_r,
                                            relu, y, y16, ld_y, None)


def test_the_export_agrees_with_the_header_and_the_binding():
    import ctypes
    from csn_amd import _lib
    _lib.build()
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"CSN_API int " + NAME + r"\(([^;]*)\);", header)
    assert m, "the header does not declare the entry point"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "x", "x16", "ld_x", "n_in", "table", "n_out", "kv", "c_in", "c_out", "w", "gamma", "beta", "running_mean", "running_var", "eps",
        "r", "r16", "ld_r", "relu", "y", "y16", "ld_y", "stream"]
    kinds = {"*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float}
    want = [kinds["*"] if "*" in p else kinds[" ".join(p.split()[:-1]).replace("const ", "")] for p in params]
    res, args = _lib._SIGNATURES[NAME]
    assert res is ctypes.c_int and args == want
    assert "(24)" in header and header.index("(24)") > header.index("(23)")
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NAME + r"\b", names), "libcsn_hip.so does not export the entry point"
    assert NAME in _lib.EXPORTS and "sparse_conv_maps16.hip" in _lib.SOURCES and _lib.lib().csn_version() == 17


def test_section_24_rejects_bad_arguments_on_the_host(lib16):
    f = lambda **kw: _f(lib16, **kw)
    # a call whose arguments are all valid gets past every check but the last one tried here: a misaligned x
    assert f(x=FAKE + 4) == PTR
    for name in ("x", "table", "w", "gamma", "beta", "rm", "rv", "y"):
        assert f(**{name: None}) == ARG, name
    for flag in ("x16", "r16", "y16"):
        assert f(**{flag: 2}) == ARG and f(**{flag: -1}) == ARG, flag
    assert f(n_in=0) == ARG and f(n_out=0) == ARG
    assert f(kv=8) == DIM and f(c_in=40, ld_x=40) == DIM and f(c_out=288, ld_y=288, ld_r=288) == DIM
    assert f(c_in=288, ld_x=288) == DIM and f(c_out=40, ld_y=40, ld_r=40) == DIM and f(c_in=0) == DIM
    # 16-bit pitches: % 8, at least the width, at most 2^20, and the map inside the 2 GiB window at 2 bytes an element
    assert f(ld_x=68) == ALIGN and f(ld_y=36) == ALIGN and f(ld_r=36) == ALIGN
    assert f(ld_x=56) == ARG and f(ld_y=24) == ARG and f(ld_r=24) == ARG
    assert f(ld_x=(1 << 20) + 8) == DIM and f(ld_y=(1 << 20) + 8) == DIM and f(ld_r=(1 << 20) + 8) == DIM
    assert f(n_in=1 << 25) == DIM and f(n_out=1 << 26) == DIM
    assert f(n_out=1 << 22, ld_y=480, r=None) == DIM and f(n_out=1 << 22, ld_y=32, ld_r=480) == DIM
    # alignment: 16 bytes whatever the map's type
    assert f(x=FAKE + 8) == PTR and f(w=FAKE + 8) == PTR and f(y=FAKE + 8) == PTR and f(r=OTHER + 8) == PTR and f(table=FAKE + 2) == PTR
    assert f(x16=0, x=FAKE + 4) == PTR and f(y16=0, y=FAKE + 4) == PTR and f(r16=0, r=OTHER + 4) == PTR
    # the residual: ignored when NULL (its pitch and its flag's map check with it)
    assert f(r=None, ld_r=0, ld_y=24) == ARG and f(r=None, ld_r=3, x=FAKE + 4) == PTR


def test_the_two_element_sizes_are_checked_side_by_side(lib16):
    f = lambda **kw: _f(lib16, **kw)
    # pitch % 8 for the 16-bit map, % 4 for the fp32 map of the same call
    assert f(x16=0, ld_x=68, y16=1, ld_y=36) == ALIGN                       # x passes (% 4), y fails (% 8)
    assert f(x16=0, ld_x=68, x=FAKE + 4) == PTR and f(x16=1, ld_x=68, x=FAKE + 4) == ALIGN
    assert f(y16=0, ld_y=36, r16=0, ld_r=36, x=FAKE + 4) == PTR and f(y16=0, ld_y=36, r16=1, ld_r=36) == ALIGN
    assert f(x16=0, ld_x=66) == ALIGN and f(y16=0, ld_y=34) == ALIGN and f(r16=0, ld_r=34) == ALIGN
    # the window: rows * pitch * 2 for a 16-bit map, * 4 for an fp32 map — 2^21 rows of 480 elements fit the first alone
    n = 1 << 21
    assert n * 480 * 2 <= 0x7fffffff < n * 480 * 4
    assert f(n_out=n, ld_y=480, y16=1, r=None, x=FAKE + 4) == PTR and f(n_out=n, ld_y=480, y16=0, r=None, x=FAKE + 4) == DIM
    assert f(n_out=n, r16=1, ld_r=480, x=FAKE + 4) == PTR and f(n_out=n, r16=0, ld_r=480, x=FAKE + 4) == DIM
    assert f(n_in=n, c_in=256, ld_x=480, x16=1, x=FAKE + 4) == PTR and f(n_in=n, c_in=256, ld_x=480, x16=0, x=FAKE + 4) == DIM
    # all flags 0 is a valid call shape: (19)'s checks
    assert f(x16=0, r16=0, y16=0, x=FAKE + 4) == PTR and f(x16=0, r16=0, y16=0, ld_r=34) == ALIGN


def test_the_aliasing_rule_with_mixed_types(lib16):
    f = lambda **kw: _f(lib16, **kw)
    # r == y passes only with the same type AND the same pitch (the misaligned x is the check behind the aliasing rule)
    assert f(r=FAKE, ld_r=64, ld_y=64, x=FAKE + 4) == PTR
    assert f(r=FAKE, r16=0, y16=0, ld_r=64, ld_y=64, x=FAKE + 4) == PTR
    assert f(r=FAKE, ld_r=64, ld_y=32) == ARG and f(r=FAKE, ld_r=32, ld_y=64) == ARG
    assert f(r=FAKE, r16=0, y16=1, ld_r=32, ld_y=32) == ARG and f(r=FAKE, r16=1, y16=0, ld_r=32, ld_y=32) == ARG
    # different pointers may mix types freely
    assert f(r=OTHER, r16=0, y16=1, x=FAKE + 4) == PTR and f(r=OTHER, r16=1, y16=0, x=FAKE + 4) == PTR


def test_section_24_needs_a_single_product_mode():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    try:
        for mode, rows16, want in ((0, 1, ARG), (1, 1, ARG), (2, 0, ARG), (3, 0, ARG), (2, 1, PTR), (3, 1, PTR)):
            L.csn_set_thread_math_mode(mode)
            L.csn_set_thread_rows16(rows16)
            # valid but for a misaligned x: PTR where the mode admits the call, ARG before any other check where it does not
            assert _f(L, x=FAKE + 4) == want, (mode, rows16)
            assert _f(L, x16=0, r16=0, y16=0, x=FAKE + 4) == want, (mode, rows16)
    finally:
        L.csn_set_thread_rows16(0)
        L.csn_set_thread_math_mode(-1)


def test_the_switch_defaults_to_off_and_round_trips():
    from csn_amd import tuning
    assert tuning.Tuning().infer_maps16 is False and tuning.current().infer_maps16 is False
    with tuning.override(infer_maps16=True) as t:
        assert t.infer_maps16 is True and tuning.current().infer_maps16 is True
        with tuning.override(infer_maps16=False):
            assert tuning.current().infer_maps16 is False
        assert tuning.current().infer_maps16 is True
    assert tuning.current().infer_maps16 is False


def test_python_route_refuses_cpu_tensors_and_16_bit_tensors_without_the_mode():
    from csn_amd import CsnError, build_pyramid, maps16_dtype, sparse_conv_bn_act, tuning
    from csn_amd import functional as CF
    kmap = build_pyramid(torch.tensor(R.dense_block()), 2).s1[0]
    w, norm = torch.zeros(27, 32, 32), torch.nn.BatchNorm1d(32)
    x32 = torch.zeros(64, 32)
    with pytest.raises(CsnError):
        sparse_conv_bn_act(x32, w, kmap, norm)
    # a 16-bit tensor (or an out_dtype) without the mode, or without the switch
    assert maps16_dtype() is None
    with pytest.raises(ValueError, match="rows_single_product"):
        sparse_conv_bn_act(x32.bfloat16(), w, kmap, norm)
    with pytest.raises(ValueError, match="rows_single_product"):
        sparse_conv_bn_act(x32, w, kmap, norm, out_dtype=torch.bfloat16)
    with CF.math_mode("bf16"), pytest.raises(ValueError, match="rows_single_product"):
        sparse_conv_bn_act(x32, w, kmap, norm, residual=torch.zeros(64, 32).bfloat16())
    with tuning.override(rows_single_product=True):
        for mode in ("fp32", "bf16x3"):
            with CF.math_mode(mode), pytest.raises(ValueError, match="math mode"):
                sparse_conv_bn_act(x32.half(), w, kmap, norm)
        # the mode and the switch, and a tensor of the other 16-bit type
        with CF.math_mode("bf16"):
            assert maps16_dtype() is torch.bfloat16
            with pytest.raises(ValueError, match="float16"):
                sparse_conv_bn_act(x32.half(), w, kmap, norm)
            with pytest.raises(ValueError, match="float16"):
                sparse_conv_bn_act(x32, w, kmap, norm, out_dtype=torch.float16)
            with pytest.raises(ValueError, match="out_dtype"):
                sparse_conv_bn_act(x32, w, kmap, norm, out=torch.zeros(64, 32), out_dtype=torch.bfloat16)
            with pytest.raises(CsnError):                                   # the route is open: CPU tensors are what is left
                sparse_conv_bn_act(x32.bfloat16(), w, kmap, norm)
        with CF.math_mode("fp16"):
            assert maps16_dtype() is torch.float16
            with pytest.raises(ValueError, match="bfloat16"):
                sparse_conv_bn_act(x32.bfloat16(), w, kmap, norm)
            with pytest.raises(CsnError):
                sparse_conv_bn_act(x32, w, kmap, norm, out_dtype=torch.float16)
    assert maps16_dtype() is None


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_round16_is_the_cpu_cast_and_idempotent(kind):
    g = torch.Generator().manual_seed(5)
    t = torch.cat([torch.randn(4096, generator=g), 1e-3 * torch.randn(4096, generator=g), 300.0 * torch.randn(4096, generator=g),
                   torch.tensor([0.0, -0.0, 1.0, 65504.0, 65519.0, 65520.0, 1e5, -1e5, 2.0 ** -14, 2.0 ** -24, 1.0 + 2.0 ** -8,
                                 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])])
    dtype = R16.DTYPES[kind]
    r = R16.round16(t, kind)
    assert r.dtype == torch.float32 and torch.equal(r, t.to(dtype).float())
    assert torch.equal(R16.round16(r, kind), r) and torch.equal(r.to(dtype).float(), r)
    # ties go to even; an fp16 overflow is inf (a plain conversion, not a clamp)
    one = lambda v: R16.round16(torch.tensor([v]), kind).item()
    if kind == "fp16":
        assert one(1.0 + 2.0 ** -11) == 1.0 and one(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9 and one(65520.0) == float("inf")
    else:
        assert one(1.0 + 2.0 ** -8) == 1.0 and one(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6 and one(1e5) == 99840.0


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_maps16_instances_keep_registers_lds_and_occupancy(tmp_path):
    """NB 1..4 x (bf16, fp16) x (fp32 A, 16-bit A): no scratch, no spilled vector registers, the B tile of NB * 32 columns x 40
    shorts plus the offset lists in LDS, and at least the waves per SIMD of ``sconv_gemm16_bn_kernel<NB, H16>`` in the same compile."""
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    sources = ["sparse_conv_maps16.hip", "sparse_conv.hip"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in sources]
    new, old = {}, {}
    for proc in procs:
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            # (anonymous namespace)::sconv_maps16_kernel<NB, H16, A16> / ::sconv_gemm16_bn_kernel<NB, H16>
            m = re.match(r"_ZN12_GLOBAL__N_1\d+sconv_maps16_kernelILi(\d)ELb(\d)ELb(\d)EE", b)
            if m:
                nb, h16, a16 = (int(v) for v in m.groups())
                assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0, m.group(0)
                assert field("LDS Size [bytes/block]") <= nb * 32 * 40 * 2 + 1012, m.group(0)
                new[(nb, h16, a16)] = field("Occupancy [waves/SIMD]")
                continue
            m = re.match(r"_ZN12_GLOBAL__N_1\d+sconv_gemm16_bn_kernelILi(\d)ELb(\d)EE", b)
            if m:
                old[(int(m.group(1)), int(m.group(2)))] = field("Occupancy [waves/SIMD]")
    assert sorted(new) == [(nb, h, a) for nb in (1, 2, 3, 4) for h in (0, 1) for a in (0, 1)]
    assert sorted(old) == [(nb, h) for nb in (1, 2, 3, 4) for h in (0, 1)]
    for (nb, h16, a16), waves in new.items():
        assert waves >= old[(nb, h16)], ((nb, h16, a16), waves, old[(nb, h16)])
