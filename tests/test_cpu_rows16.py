"""CPU-side checks (no GPU needed) of the single-product row products (csn_set_thread_rows16; tuning.rows_single_product): the
thread flag and the tuning switch; every single-product instance of the four matrix kernels built on csrc/rows_mma.h —
rows_gemm16 / rows_fc_wgrad16 (csrc/rows_fc.hip), sconv_gemm16 / sconv_wgrad16 (csrc/sparse_conv.hip) — compiles for gfx950 without
scratch memory and without spilled vector registers, in no more LDS than the bf16x3 instance of the same NB / TA (and B layout), and
at no fewer waves per SIMD than the floor tests/test_cpu_rows_mma_resources.py sets for math mode 1 at that NB / TA; and the
reference helper tests/rows16_ref.py on hand-written values."""
import os
import re
import subprocess
import threading

import pytest
import torch

from tests import rows16_ref as R16
from tests import sparse_conv_ref as R
from tests.test_cpu_rows_mma_resources import GEMM_WAVES, ROOT, WGRAD_WAVES, _hipcc

SOURCES = ["rows_fc.hip", "sparse_conv.hip"]
# forward products in bf16 and fp16 at NB 1..4 plus the bf16 dx product (rows_gemm16: NB 4 on [K][J] weights; sconv_gemm16: NB 1..4
# on [J][K]); the weight gradients in bf16 at TA 1..4
INSTANCES = {"rows_gemm16_kernel": 9, "sconv_gemm16_kernel": 12, "rows_fc_wgrad16_kernel": 4, "sconv_wgrad16_kernel": 4}
X3 = {"rows_gemm16_kernel": "rows_gemm_kernel", "sconv_gemm16_kernel": "sconv_gemm_kernel", "rows_fc_wgrad16_kernel": "rows_fc_wgrad_kernel",
      "sconv_wgrad16_kernel": "sconv_wgrad_kernel"}


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


def test_thread_flag(L):
    lib = L.lib()
    assert lib.csn_get_thread_rows16() == 0
    try:
        assert lib.csn_set_thread_rows16(1) == 0 and lib.csn_get_thread_rows16() == 1
        for bad in (2, -1):
            assert lib.csn_set_thread_rows16(bad) == -1 and lib.csn_get_thread_rows16() == 1
        seen = []
        t = threading.Thread(target=lambda: seen.append(lib.csn_get_thread_rows16()))
        t.start()
        t.join()
        assert seen == [0] and lib.csn_get_thread_rows16() == 1
    finally:
        assert lib.csn_set_thread_rows16(0) == 0
    assert lib.csn_version() == 17


def test_context_manager_and_tuning_switch(L):
    from csn_amd import functional as CF
    from csn_amd import tuning
    lib = L.lib()
    with CF.rows16(True):
        assert lib.csn_get_thread_rows16() == 1
        with CF.rows16(False):
            assert lib.csn_get_thread_rows16() == 0
        assert lib.csn_get_thread_rows16() == 1
    assert lib.csn_get_thread_rows16() == 0
    assert tuning.Tuning().rows_single_product is False and tuning.current().rows_single_product is False
    with tuning.override(rows_single_product=True):
        assert tuning.current().rows_single_product is True
        with tuning.override(rows_single_product=False):
            assert tuning.current().rows_single_product is False
        assert tuning.current().rows_single_product is True
    assert tuning.current().rows_single_product is False


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_single_product_instances_keep_registers_lds_and_occupancy(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in SOURCES]
    new, x3_lds = [], {}
    for proc in procs:
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            field = lambda key, b=b: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            # NAME16<NB, H16, B_KN> / NAME16<TA>, and the bf16x3 instances NAME<NB, 1, B_KN> / NAME<TA, 1> they are held against
            m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?16_kernel)ILi(\d)E(?:Lb(\d)ELb(\d)E)?E", b)
            if m and m.group(1) in INSTANCES:
                new.append((m.group(1), int(m.group(2)), m.group(3), m.group(4), field))
                continue
            m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)ILi(\d)ELi1E(?:Lb(\d)E)?E", b)
            if m and m.group(1) in X3.values():
                x3_lds[(m.group(1), int(m.group(2)), m.group(3))] = field("LDS Size [bytes/block]")
    seen = dict.fromkeys(INSTANCES, 0)
    for kernel, n, h16, b_kn, field in new:
        name = f"{kernel}<{n}" + (f", {h16}, {b_kn}>" if h16 is not None else ">")
        assert field("ScratchSize [bytes/lane]") == 0, name
        assert field("VGPRs Spill") == 0, name
        assert field("LDS Size [bytes/block]") <= x3_lds[(X3[kernel], n, b_kn)], name
        floor = (GEMM_WAVES if h16 is not None else WGRAD_WAVES)[X3[kernel]][1][n - 1]
        assert field("Occupancy [waves/SIMD]") >= floor, name
        seen[kernel] += 1
    assert seen == INSTANCES


def test_round16_on_hand_written_values():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    # bf16 keeps 8 significant bits: 1 + 2^-8 and 1 + 3 2^-8 are ties (to the even neighbours 1 and 1 + 2^-6); 2 - 2^-9 rounds up
    # across the power of two; 1 + 2^-8 + 2^-20 is past the tie
    got = R16.round16(t(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2 - 2.0 ** -9, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 3 * 2.0 ** -8), 0.0), "bf16")
    assert got.dtype == torch.float32
    assert got.tolist() == [1.0, 1 + 2.0 ** -6, 2.0, 1 + 2.0 ** -7, -(1 + 2.0 ** -6), 0.0]
    # fp16 keeps 11
    got = R16.round16(t(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2 - 2.0 ** -13, 1 + 2.0 ** -11 + 2.0 ** -22, 2.0 ** -14), "fp16")
    assert got.tolist() == [1.0, 1 + 2.0 ** -9, 2.0, 1 + 2.0 ** -10, 2.0 ** -14]
    z = R16.no_subnormals(t(2.0 ** -14, -2.0 ** -15, 3e-5, 1.0, 0.0))
    assert z.tolist() == [2.0 ** -14, 0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_conv_restatement(kind):
    """Forward: ``R.fwd`` on operands rounded to ``kind``; gradients through autograd: ``R.bwd`` on bf16-rounded dy, x and w."""
    g, _ = R.geometry("s1", R.random_set(33))
    t = R.tensors(3, g.n_in, g.n_out, g.KV, 32, 64)
    x, w = t["x"].double().requires_grad_(True), t["w"].double().requires_grad_(True)
    y = R16.conv(kind)(g, x, w)
    assert y.dtype == torch.float64 and torch.equal(y.detach(), R.fwd(g, R16.round16(t["x"], kind), R16.round16(t["w"], kind)))
    assert not torch.equal(y.detach(), R.fwd(g, t["x"], t["w"]))
    dx, dw = torch.autograd.grad(y, [x, w], t["dy"].double())
    b = R.bwd(g, R16.round16(t["dy"], "bf16"), R16.round16(t["x"], "bf16"), R16.round16(t["w"], "bf16"))
    assert torch.equal(dx, b["dx"]) and torch.equal(dw, b["dw"])
