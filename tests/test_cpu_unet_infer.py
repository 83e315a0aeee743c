"""The Res16UNets' inference graph (csn_amd/minkowski_unet.py; include/csn_hip.h section 23), checked without a GPU: the two new
exports against the header and the ctypes binding; every host-side argument check of ``csn_octant_down_bn_act_fwd_f32`` and
``csn_octant_up_bn_act_fwd_f32`` (the codes of section 21, plus section 19's for the residual); the registers, LDS and waves per SIMD
of the eight BN instances of ``octant_rows_kernel`` beside their plain neighbours in one compile; the refusals (CPU tensors, a layer
with a bias, the ``REFUSED`` classes)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import sparse_conv_ref as R

DOWN, UP = "csn_octant_down_bn_act_fwd_f32", "csn_octant_up_bn_act_fwd_f32"
TAIL = ["gamma", "beta", "running_mean", "running_var", "eps", "r", "ld_r", "relu", "y", "ld_y", "stream"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN, PTR, DIM = -1, -2, -3, -5


# ------------------------------------------------------------------------------------------------------
# the exports
# ------------------------------------------------------------------------------------------------------
def _params(header, name):
    m = re.search(r"CSN_API int " + name + r"\(([^;]*)\);", header)
    assert m, f"the header does not declare {name}"
    return [p.strip() for p in m.group(1).replace("\n", " ").split(",")]


def test_the_new_exports_agree_with_the_header_and_the_binding():
    from csn_amd import _lib
    _lib.build()
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as fh:
        header = fh.read()
    names_of = lambda ps: [p.split()[-1].lstrip("*") for p in ps]
    # the map arguments of section 21 without bias, then section 19's tail
    for new, old in ((DOWN, "csn_octant_down_fwd_f32"), (UP, "csn_octant_up_fwd_f32")):
        params = _params(header, new)
        plain = [p for p in names_of(_params(header, old)) if p not in ("bias", "y", "ld_y", "stream")]
        assert names_of(params) == plain + TAIL, new
        assert names_of(_params(header, "csn_sparse_conv_bn_act_fwd_f32"))[-len(TAIL):] == TAIL
        kinds = {"*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float}
        want = [kinds["*"] if "*" in p else kinds[" ".join(p.split()[:-1]).replace("const ", "")] for p in params]
        res, args = _lib._SIGNATURES[new]
        assert res is ctypes.c_int and args == want, new
        assert new in _lib.EXPORTS
    assert "(23)" in header and header.index("(23)") > header.index("(22)")
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for new in (DOWN, UP):
        assert re.search(r"\bT " + new + r"\b", names), f"libcsn_hip.so does not export {new}"
    assert _lib.lib().csn_version() == 17


# ------------------------------------------------------------------------------------------------------
# host-side argument checks of section 23
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_section_23_rejects_bad_arguments_on_the_host(up):
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    FAKE, OTHER = 1 << 20, 1 << 22

    # (every call below fails a check: nothing is ever launched on these made-up addresses)
    def f(x=FAKE, ld_x=64, n_fine=13, n_coarse=11, children=FAKE, parent=FAKE, order=FAKE, seg=FAKE, c_in=64, c_out=32, w=FAKE,
          gamma=FAKE, beta=FAKE, rm=FAKE, rv=FAKE, r=OTHER, ld_r=32, relu=1, y=FAKE, ld_y=32):
        tail = (w, gamma, beta, rm, rv, 1e-5, r, ld_r, relu, y, ld_y, None)
        if up:
            return L.csn_octant_up_bn_act_fwd_f32(x, ld_x, n_coarse, parent, order, seg, n_fine, c_in, c_out, *tail)
        return L.csn_octant_down_bn_act_fwd_f32(x, ld_x, n_fine, children, n_coarse, c_in, c_out, *tail)
    n_x, n_y = ("n_coarse", "n_fine") if up else ("n_fine", "n_coarse")    # the rows of x; of y and r
    for name in ("x", "w", "gamma", "beta", "rm", "rv", "y") + (("parent", "order", "seg") if up else ("children",)):
        assert f(**{name: None}) == ARG, name
    assert f(n_fine=0) == ARG and f(n_coarse=0) == ARG and f(n_fine=-3) == ARG
    # widths 0 / 40 / 288
    assert f(c_in=0) == DIM and f(c_in=40, ld_x=40) == DIM and f(c_in=288, ld_x=288) == DIM
    assert f(c_out=0) == DIM and f(c_out=40, ld_y=40, ld_r=40) == DIM and f(c_out=288, ld_y=288, ld_r=288) == DIM
    # pitches: % 4, at least the width, at most 2^20, and the map inside the 2 GiB window
    assert f(ld_x=66) == ALIGN and f(ld_y=34) == ALIGN and f(ld_r=34) == ALIGN
    assert f(ld_x=60) == ARG and f(ld_y=28) == ARG and f(ld_r=28) == ARG
    assert f(ld_x=(1 << 20) + 4) == DIM and f(ld_y=(1 << 20) + 4) == DIM and f(ld_r=(1 << 20) + 4) == DIM
    assert f(**{n_x: 1 << 24}) == DIM and f(**{n_y: 1 << 24}) == DIM
    assert f(**{n_y: 1 << 21}, ld_y=480, r=None) == DIM and f(**{n_y: 1 << 21}, ld_y=32, ld_r=480) == DIM
    assert f(**{n_x: 1 << 21}, ld_x=480) == DIM
    # alignment
    assert f(x=FAKE + 4) == PTR and f(w=FAKE + 8) == PTR and f(y=FAKE + 4) == PTR and f(r=OTHER + 8) == PTR
    for name in (("parent", "order", "seg") if up else ("children",)):
        assert f(**{name: FAKE + 2}) == PTR, name
    # the residual: ignored when NULL (its pitch with it); y itself only element for element
    assert f(r=None, ld_r=0, ld_y=28) == ARG and f(r=None, ld_r=3, x=FAKE + 4) == PTR
    assert f(r=FAKE, ld_r=64, ld_y=32) == ARG and f(r=FAKE, ld_r=32, ld_y=64) == ARG
    assert f(r=FAKE, ld_r=64, ld_y=64, x=FAKE + 4) == PTR                   # r == y at one pitch passes the aliasing rule


def test_sections_19_and_21_refuse_what_they_refused():
    """Section 23 is additive: section 19 still takes no table of 8 offsets and no width above 256, section 21 keeps its codes."""
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    F = 1 << 20
    s19 = lambda kv=27, c_in=64, ld_x=64: L.csn_sparse_conv_bn_act_fwd_f32(F, ld_x, 13, F, 11, kv, c_in, 32, F, F, F, F, F, 1e-5, None, 0, 1,
                                                                           F, 32, None)
    assert s19(kv=8) == DIM and s19(c_in=288, ld_x=288) == DIM
    assert L.csn_octant_down_fwd_f32(F, 64, 13, F, 11, 64, 288, F, None, F, 288, None) == DIM
    assert L.csn_octant_up_fwd_f32(F, 64, 11, F, F, F + 2, 13, 64, 32, F, None, F, 32, None) == PTR


# ------------------------------------------------------------------------------------------------------
# the new instances' resources
# ------------------------------------------------------------------------------------------------------
def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_the_bn_instances_cost_no_more_than_their_plain_neighbours(tmp_path):
    """Every ``octant_rows_bn_kernel<NB, MODE>`` beside ``octant_rows_kernel<NB, MODE, true>`` in the same compile: no scratch, no
    spilled registers, no more LDS, no fewer waves per SIMD."""
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                               os.path.join(ROOT, "csn_amd", "csrc", "octant_conv.hip"), "-o", str(tmp_path / "octant_conv.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    plain, bn = {}, {}
    for b in re.split(r"Function Name: ", res.stderr)[1:]:
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        # (anonymous namespace)::octant_rows[_bn]_kernel<int, int[, bool]>
        m = re.match(r"_ZN12_GLOBAL__N_1\d+octant_rows(_bn)?_kernelILi(\d)ELi(\d)E(?:Lb(\d)E)?E", b)
        if not m:
            continue
        key = (int(m.group(2)), int(m.group(3)))
        figures = {q: field(q) for q in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
                                         "Occupancy [waves/SIMD]", "VGPRs", "AGPRs", "SGPRs")}
        if m.group(1):
            bn[key] = figures
        elif m.group(4) == "1":
            plain[key] = figures
    want = {(nb, mode) for nb in (1, 2, 3, 4) for mode in (0, 1)}
    assert set(bn) == want and set(plain) == want
    for key in sorted(want):
        b, p = bn[key], plain[key]
        print(f"[unet-infer] octant_rows_bn_kernel<{key[0]}, {key[1]}>: {b['VGPRs']} + {b['AGPRs']} VGPR / {b['SGPRs']} SGPR / "
              f"{b['LDS Size [bytes/block]']} B LDS / {b['Occupancy [waves/SIMD]']} waves (plain: {p['VGPRs']} + {p['AGPRs']} / "
              f"{p['SGPRs']} / {p['LDS Size [bytes/block]']} / {p['Occupancy [waves/SIMD]']})")
        assert b["ScratchSize [bytes/lane]"] == 0 and b["VGPRs Spill"] == 0 and b["SGPRs Spill"] == 0, key
        assert b["LDS Size [bytes/block]"] <= p["LDS Size [bytes/block]"], key
        assert b["Occupancy [waves/SIMD]"] >= p["Occupancy [waves/SIMD]"], key


# ------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_biased_layers_are_refused():
    import csn_amd
    from csn_amd import CsnError, Res16UNet14A, build_octant_map, octant_conv_bn_act, tuning
    from csn_amd import minkowski_unet as MU
    from csn_amd.minkowski_conv import SparseConvDown2, SparseConvUp2
    pts = torch.tensor(R.dense_block())
    omap = build_octant_map(pts)
    norm = torch.nn.BatchNorm1d(32)
    for up, n in ((False, omap.n_fine), (True, omap.n_coarse)):
        with pytest.raises(CsnError):
            octant_conv_bn_act(torch.zeros(n, 32), torch.zeros(8, 32, 32), omap, norm, up)
    # a layer with a bias is refused before anything else; the U-Nets have none
    for cls in (SparseConvDown2, SparseConvUp2):
        with pytest.raises(ValueError, match="bias"):
            MU._octant_bn_act(cls(32, 32, bias=True), norm, torch.zeros(omap.n_fine, 32), omap)
    model = Res16UNet14A(3, 5).eval()
    assert all(getattr(m, "bias", None) is None for m in model.modules() if isinstance(m, SparseConvDown2))
    with torch.no_grad(), tuning.override(eval_epilogue=True), pytest.raises(CsnError):
        model((pts, torch.zeros(pts.shape[0], 3)))
    with torch.no_grad(), tuning.override(eval_epilogue=True), pytest.raises(CsnError):
        model.block5[0].infer(torch.zeros(4, 256), None, None)
    assert csn_amd.octant_conv_bn_act is octant_conv_bn_act


def test_the_refused_classes_are_still_refused():
    import csn_amd
    from csn_amd.minkowski_unet import REFUSED
    assert REFUSED == ("Res16UNet14D", "Res16UNet18D", "Res16UNet50", "Res16UNet101")
    for name in REFUSED:
        with pytest.raises(NotImplementedError):
            getattr(csn_amd, name)(3, 5)
