"""The Res16UNets' single-product octant launches on 16-bit maps (include/csn_hip.h section 25, csn_amd/csrc/octant_conv_maps16.hip,
``tuning.octant_single_product`` / ``tuning.unet_maps16``), checked without a GPU: header, binding and export of the two entry
points; every host-side argument check of both with made-up pointers (nothing is launched); the two switches; the Python route's
refusals; and the resources of the sixteen UP kernel instances against the ``octant_rows_bn_kernel<NB, 1>`` instance of the same
column blocks, read from the same compile."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import sparse_conv_ref as R

DOWN, UP = "csn_octant_down_bn_act_fwd_m16", "csn_octant_up_bn_act_fwd_m16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN, PTR, DIM = -1, -2, -3, -5
FAKE, OTHER = 1 << 20, 1 << 22
TAIL = ["c_in", "c_out", "w", "gamma", "beta", "running_mean", "running_var", "eps", "r", "r16", "ld_r", "relu", "y", "y16", "ld_y", "stream"]
PARAMS = {DOWN: ["x", "x16", "ld_x", "n_fine", "children", "n_coarse"] + TAIL,
          UP: ["x", "x16", "ld_x", "n_coarse", "parent", "order", "seg", "n_fine"] + TAIL}


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


def _f(L, up, x=FAKE, x16=1, ld_x=64, n_fine=13, n_coarse=5, children=FAKE, parent=FAKE, order=FAKE, seg=FAKE, c_in=64, c_out=32, w=FAKE,
       gamma=FAKE, beta=FAKE, rm=FAKE, rv=FAKE, r=OTHER, r16=1, ld_r=32, relu=1, y=FAKE, y16=1, ld_y=32):
    # (every call below fails a check: nothing is ever launched on these made-up addresses)
    tail = (c_in, c_out, w, gamma, beta, rm, rv, 1e-5, r, r16, ld_r, relu, y, y16, ld_y, None)
    if up:
        return L.csn_octant_up_bn_act_fwd_m16(x, x16, ld_x, n_coarse, parent, order, seg, n_fine, *tail)
    return L.csn_octant_down_bn_act_fwd_m16(x, x16, ld_x, n_fine, children, n_coarse, *tail)


BOTH = pytest.mark.parametrize("up", [False, True], ids=["down", "up"])


def test_the_exports_agree_with_the_header_and_the_binding():
    from csn_amd import _lib
    _lib.build()
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as fh:
        header = fh.read()
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kinds = {"*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in (DOWN, UP):
        m = re.search(r"CSN_API int " + name + r"\(([^;]*)\);", header)
        assert m, f"the header does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == PARAMS[name]
        want = [kinds["*"] if "*" in p else kinds[" ".join(p.split()[:-1]).replace("const ", "")] for p in params]
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and args == want, name
        assert re.search(r"\bT " + name + r"\b", names), f"libcsn_hip.so does not export {name}"
        assert name in _lib.EXPORTS
    assert "(25)" in header and header.index("(25)") > header.index("(24)")
    assert "octant_conv_maps16.hip" in _lib.SOURCES and _lib.lib().csn_version() == 17
    # section 24's own entry point still refuses the 8-offset table: section 25's down launch is the door to it
    L = _lib.lib()
    try:
        L.csn_set_thread_math_mode(2)
        L.csn_set_thread_rows16(1)
        assert L.csn_sparse_conv_bn_act_fwd_m16(FAKE, 1, 64, 13, FAKE, 11, 8, 64, 32, FAKE, FAKE, FAKE, FAKE, FAKE, 1e-5, None, 0, 0, 1, FAKE, 1,
                                                32, None) == DIM
    finally:
        L.csn_set_thread_rows16(0)
        L.csn_set_thread_math_mode(-1)


@BOTH
def test_section_25_rejects_bad_arguments_on_the_host(lib16, up):
    f = lambda **kw: _f(lib16, up, **kw)
    n_x, n_y = ("n_coarse", "n_fine") if up else ("n_fine", "n_coarse")
    # a call whose arguments are all valid gets past every check but the last one tried here: a misaligned x
    assert f(x=FAKE + 4) == PTR
    for name in ("x", "w", "gamma", "beta", "rm", "rv", "y") + (("parent", "order", "seg") if up else ("children",)):
        assert f(**{name: None}) == ARG, name
    for flag in ("x16", "r16", "y16"):
        assert f(**{flag: 2}) == ARG and f(**{flag: -1}) == ARG, flag
    assert f(n_fine=0) == ARG and f(n_coarse=0) == ARG
    assert f(c_in=40, ld_x=40) == DIM and f(c_out=288, ld_y=288, ld_r=288) == DIM
    assert f(c_in=288, ld_x=288) == DIM and f(c_out=40, ld_y=40, ld_r=40) == DIM and f(c_in=0) == DIM
    # 16-bit pitches: % 8, at least the width, at most 2^20, and the map inside the 2 GiB window at 2 bytes an element
    assert f(ld_x=68) == ALIGN and f(ld_y=36) == ALIGN and f(ld_r=36) == ALIGN
    assert f(ld_x=56) == ARG and f(ld_y=24) == ARG and f(ld_r=24) == ARG
    assert f(ld_x=(1 << 20) + 8) == DIM and f(ld_y=(1 << 20) + 8) == DIM and f(ld_r=(1 << 20) + 8) == DIM
    assert f(**{n_x: 1 << 25}) == DIM and f(**{n_y: 1 << 26}) == DIM
    assert f(**{n_y: 1 << 22}, ld_y=480, r=None) == DIM and f(**{n_y: 1 << 22}, ld_y=32, ld_r=480) == DIM
    # alignment: 16 bytes whatever the map's type, 4 for the index arrays
    assert f(x=FAKE + 8) == PTR and f(w=FAKE + 8) == PTR and f(y=FAKE + 8) == PTR and f(r=OTHER + 8) == PTR
    for name in ("parent", "order", "seg") if up else ("children",):
        assert f(**{name: FAKE + 2}) == PTR, name
    assert f(x16=0, x=FAKE + 4) == PTR and f(y16=0, y=FAKE + 4) == PTR and f(r16=0, r=OTHER + 4) == PTR
    # the residual: ignored when NULL (its pitch and its flag's map check with it)
    assert f(r=None, ld_r=0, ld_y=24) == ARG and f(r=None, ld_r=3, x=FAKE + 4) == PTR


@BOTH
def test_the_two_element_sizes_are_checked_side_by_side(lib16, up):
    f = lambda **kw: _f(lib16, up, **kw)
    n_x, n_y = ("n_coarse", "n_fine") if up else ("n_fine", "n_coarse")
    # pitch % 8 for the 16-bit map, % 4 for the fp32 map of the same call
    assert f(x16=0, ld_x=68, y16=1, ld_y=36) == ALIGN                       # x passes (% 4), y fails (% 8)
    assert f(x16=0, ld_x=68, x=FAKE + 4) == PTR and f(x16=1, ld_x=68, x=FAKE + 4) == ALIGN
    assert f(y16=0, ld_y=36, r16=0, ld_r=36, x=FAKE + 4) == PTR and f(y16=0, ld_y=36, r16=1, ld_r=36) == ALIGN
    assert f(x16=0, ld_x=66) == ALIGN and f(y16=0, ld_y=34) == ALIGN and f(r16=0, ld_r=34) == ALIGN
    # the window: rows * pitch * 2 for a 16-bit map, * 4 for an fp32 map — 2^21 rows of 480 elements fit the first alone
    n = 1 << 21
    assert n * 480 * 2 <= 0x7fffffff < n * 480 * 4
    assert f(**{n_y: n}, ld_y=480, y16=1, r=None, x=FAKE + 4) == PTR and f(**{n_y: n}, ld_y=480, y16=0, r=None, x=FAKE + 4) == DIM
    assert f(**{n_y: n}, r16=1, ld_r=480, x=FAKE + 4) == PTR and f(**{n_y: n}, r16=0, ld_r=480, x=FAKE + 4) == DIM
    assert f(**{n_x: n}, c_in=256, ld_x=480, x16=1, x=FAKE + 4) == PTR and f(**{n_x: n}, c_in=256, ld_x=480, x16=0, x=FAKE + 4) == DIM
    # all flags 0 is a valid call shape: section 23's checks
    assert f(x16=0, r16=0, y16=0, x=FAKE + 4) == PTR and f(x16=0, r16=0, y16=0, ld_r=34) == ALIGN


@BOTH
def test_the_aliasing_rule_with_mixed_types(lib16, up):
    f = lambda **kw: _f(lib16, up, **kw)
    # r == y passes only with the same type AND the same pitch (the misaligned x is the check behind the aliasing rule)
    assert f(r=FAKE, ld_r=64, ld_y=64, x=FAKE + 4) == PTR
    assert f(r=FAKE, r16=0, y16=0, ld_r=64, ld_y=64, x=FAKE + 4) == PTR
    assert f(r=FAKE, ld_r=64, ld_y=32) == ARG and f(r=FAKE, ld_r=32, ld_y=64) == ARG
    assert f(r=FAKE, r16=0, y16=1, ld_r=32, ld_y=32) == ARG and f(r=FAKE, r16=1, y16=0, ld_r=32, ld_y=32) == ARG
    # different pointers may mix types freely
    assert f(r=OTHER, r16=0, y16=1, x=FAKE + 4) == PTR and f(r=OTHER, r16=1, y16=0, x=FAKE + 4) == PTR


@BOTH
def test_section_25_needs_a_single_product_mode(up):
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    try:
        for mode, rows16, want in ((0, 1, ARG), (1, 1, ARG), (2, 0, ARG), (3, 0, ARG), (2, 1, PTR), (3, 1, PTR)):
            L.csn_set_thread_math_mode(mode)
            L.csn_set_thread_rows16(rows16)
            # valid but for a misaligned x: PTR where the mode admits the call, ARG before any other check where it does not
            assert _f(L, up, x=FAKE + 4) == want, (mode, rows16)
            assert _f(L, up, x16=0, r16=0, y16=0, x=FAKE + 4) == want, (mode, rows16)
    finally:
        L.csn_set_thread_rows16(0)
        L.csn_set_thread_math_mode(-1)


def test_the_switches_default_to_off_and_nest():
    from csn_amd import tuning
    for name in ("octant_single_product", "unet_maps16"):
        assert getattr(tuning.Tuning(), name) is False and getattr(tuning.current(), name) is False
    with tuning.override(unet_maps16=True) as t:
        assert t.unet_maps16 is True and t.octant_single_product is False and tuning.current().infer_maps16 is False
        with tuning.override(octant_single_product=True, unet_maps16=False):
            assert tuning.current().octant_single_product is True and tuning.current().unet_maps16 is False
            with tuning.override(infer_maps16=True):
                assert tuning.current().octant_single_product is True and tuning.current().unet_maps16 is False
        assert tuning.current().unet_maps16 is True and tuning.current().octant_single_product is False
    assert tuning.current().unet_maps16 is False and tuning.current().octant_single_product is False


@BOTH
def test_python_route_refuses_cpu_tensors_and_16_bit_use_without_the_mode(up):
    from csn_amd import CsnError, build_octant_map, maps16_dtype, octant_conv_bn_act, tuning
    from csn_amd import functional as CF
    omap = build_octant_map(torch.tensor(R.dense_block()))
    n_in, n_out = (omap.n_coarse, omap.n_fine) if up else (omap.n_fine, omap.n_coarse)
    w, norm = torch.zeros(8, 32, 32), torch.nn.BatchNorm1d(32)
    x32, r32 = torch.zeros(n_in, 32), torch.zeros(n_out, 32)
    call = lambda x, *a, **kw: octant_conv_bn_act(x, w, omap, norm, up, *a, **kw)
    with pytest.raises(CsnError):                                          # section 23 as ever: CPU tensors are what is wrong
        call(x32)
    # a 16-bit tensor, an out_dtype or single_product without the mode, or without the switch
    assert maps16_dtype() is None
    with pytest.raises(ValueError, match="rows_single_product"):
        call(x32.bfloat16())
    with pytest.raises(ValueError, match="rows_single_product"):
        call(x32, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rows_single_product"):
        call(x32, single_product=True)
    with CF.math_mode("bf16"), pytest.raises(ValueError, match="rows_single_product"):
        call(x32, r32.bfloat16())
    with tuning.override(rows_single_product=True):
        for mode in ("fp32", "bf16x3"):
            with CF.math_mode(mode):
                with pytest.raises(ValueError, match="math mode"):
                    call(x32.half())
                with pytest.raises(ValueError, match="math mode"):
                    call(x32, single_product=True)
        # the mode and the switch, and a tensor of the other 16-bit type
        with CF.math_mode("bf16"):
            assert maps16_dtype() is torch.bfloat16
            with pytest.raises(ValueError, match="float16"):
                call(x32.half())
            with pytest.raises(ValueError, match="float16"):
                call(x32, out_dtype=torch.float16)
            with pytest.raises(ValueError, match="float16"):
                call(x32, None, True, r32.half(), single_product=True)
            with pytest.raises(ValueError, match="out_dtype"):
                call(x32, None, True, r32, out_dtype=torch.bfloat16)
            for route in (dict(single_product=True), dict(out_dtype=torch.float32), dict(out_dtype=torch.bfloat16)):
                with pytest.raises(CsnError):                               # the route is open: CPU tensors are what is left
                    call(x32, **route)
            with pytest.raises(CsnError):
                call(x32.bfloat16())
        with CF.math_mode("fp16"):
            assert maps16_dtype() is torch.float16
            with pytest.raises(ValueError, match="bfloat16"):
                call(x32.bfloat16())
            with pytest.raises(CsnError):
                call(x32, out_dtype=torch.float16)
    assert maps16_dtype() is None


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_up_instances_keep_registers_lds_and_occupancy(tmp_path):
    """NB 1..4 x (bf16, fp16) x (fp32 A, 16-bit A): no scratch, no spilled vector registers, the W tile of NB * 32 columns x 40 shorts
    plus the 128 destinations in LDS, and at least the waves per SIMD of ``octant_rows_bn_kernel<NB, 1>`` (the bf16x3 launch these
    replace) in the same compile."""
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    sources = ["octant_conv_maps16.hip", "octant_conv.hip"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in sources]
    new, old = {}, {}
    for proc in procs:
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            # (anonymous namespace)::octant_rows_m16_kernel<NB, H16, A16> / ::octant_rows_bn_kernel<NB, MODE>
            m = re.match(r"_ZN12_GLOBAL__N_1\d+octant_rows_m16_kernelILi(\d)ELb(\d)ELb(\d)EE", b)
            if m:
                nb, h16, a16 = (int(v) for v in m.groups())
                assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0, m.group(0)
                assert field("LDS Size [bytes/block]") <= nb * 32 * 40 * 2 + 512, m.group(0)
                new[(nb, h16, a16)] = field("Occupancy [waves/SIMD]")
                continue
            m = re.match(r"_ZN12_GLOBAL__N_1\d+octant_rows_bn_kernelILi(\d)ELi1EE", b)
            if m:
                old[int(m.group(1))] = field("Occupancy [waves/SIMD]")
    assert sorted(new) == [(nb, h, a) for nb in (1, 2, 3, 4) for h in (0, 1) for a in (0, 1)]
    assert sorted(old) == [1, 2, 3, 4]
    for (nb, h16, a16), waves in new.items():
        assert waves >= old[nb], ((nb, h16, a16), waves, old[nb])
