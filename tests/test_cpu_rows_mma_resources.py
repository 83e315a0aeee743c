"""CPU-side check (no GPU needed): every instance of the four matrix kernels built on csrc/rows_mma.h — rows_gemm and rows_fc_wgrad
(csrc/rows_fc.hip), sconv_gemm and sconv_wgrad (csrc/sparse_conv.hip) — compiles for gfx950 without scratch memory and without
spilled vector registers, inside the LDS its tiles need (the B tile of NB * 32 columns x 36 floats, plus the offset lists of the
gathered product; one wave's TA x 2 accumulator blocks for the weight gradients' wave-order reduction), and at no fewer waves per
SIMD than the table below, a floor per instance.  The shared bodies are inlined into every instance, so a change to the header
shows here for all of them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["rows_fc.hip", "sparse_conv.hip", "rows_bn_act.hip"]

# waves per SIMD by (NB or TA) - 1, per math mode (0: fp32, 1: bf16x3)
GEMM_WAVES = {"rows_gemm_kernel": {0: (6, 3, 3, 3), 1: (5, 3, 3, 3)},
              "sconv_gemm_kernel": {0: (6, 4, 3, 3), 1: (5, 4, 3, 3)}}          # the same for both B layouts
WGRAD_WAVES = {"rows_fc_wgrad_kernel": {0: (3, 2, 2, 1), 1: (3, 3, 2, 1)},
               "sconv_wgrad_kernel": {0: (3, 2, 1, 1), 1: (3, 2, 1, 1)}}
GEMM_LDS_EXTRA = {"rows_gemm_kernel": 0, "sconv_gemm_kernel": 1012}            # two offset lists of 125 ints, their count, padding
INSTANCES = {"rows_gemm_kernel": 10, "sconv_gemm_kernel": 16, "rows_fc_wgrad_kernel": 8, "sconv_wgrad_kernel": 8}


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_rows_mma_instances_keep_registers_lds_and_occupancy(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in SOURCES]
    seen = dict.fromkeys(INSTANCES, 0)
    for src, proc in zip(SOURCES, procs):
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            # (anonymous namespace)::NAME<int, int[, bool]>: _ZN12_GLOBAL__N_1<len>NAME I Li<a>E Li<b>E [Lb<c>E] E ...
            m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)ILi(\d)ELi(\d)E(?:Lb(\d)E)?E", b)
            if not m or m.group(1) not in INSTANCES:
                continue
            kernel, n, mode = m.group(1), int(m.group(2)), int(m.group(3))
            name = f"{kernel}<{n}, {mode}" + (f", {m.group(4)}>" if m.group(4) else ">")
            field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            assert field("ScratchSize [bytes/lane]") == 0, name
            assert field("VGPRs Spill") == 0, name
            if kernel in GEMM_WAVES:
                assert field("LDS Size [bytes/block]") <= n * 4608 + GEMM_LDS_EXTRA[kernel], name
                assert field("Occupancy [waves/SIMD]") >= GEMM_WAVES[kernel][mode][n - 1], name
            else:
                assert field("LDS Size [bytes/block]") <= n * 8192, name
                assert field("Occupancy [waves/SIMD]") >= WGRAD_WAVES[kernel][mode][n - 1], name
            seen[kernel] += 1
    assert seen == INSTANCES
