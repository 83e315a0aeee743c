"""CPU-side check (no GPU needed): every instance of the four matrix kernels built on csrc/rows_mma.h — rows_gemm and rows_fc_wgrad
(csrc/rows_fc.hip), sconv_gemm and sconv_wgrad (csrc/sparse_conv.hip) — compiles for gfx950 without scratch memory and without
spilled vector registers, inside the LDS its tiles need (the B tile of NB * 32 columns x 36 floats, plus the offset lists of the
gathered product; one wave's TA x 2 accumulator blocks for the weight gradients' wave-order reduction), and at no fewer waves per
SIMD than the table below, a floor per instance.  The shared bodies are inlined into every instance, so a change to the header
shows here for all of them.

csrc/rows_bn_act.hip states the backward's passes and the two merges once; the backward and its sums are templates on GROUPED (false:
the whole map, true: row groups), the forward and the statistics merge have a kernel for each: no instance uses scratch or spills, and none runs at fewer waves per SIMD than the kernel it replaced did when the two were
separate copies (profiles/rows_bn_act_isa_diff.txt records those figures)."""
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
# waves per SIMD of the separate whole-map and row-group kernels before they became two instances of one body
BN_WAVES = {"rows_bn_act_fwd_kernel": 7, "rows_bn_act_groups_fwd_kernel": 5,
            "rows_bn_act_bwd_kernel<1, false>": 4, "rows_bn_act_bwd_kernel<1, true>": 4,
            "rows_bn_act_bwd_kernel<2, false>": 5, "rows_bn_act_bwd_kernel<2, true>": 4,
            "rows_bn_act_sums_kernel<false>": 8, "rows_bn_act_sums_kernel<true>": 8,
            "bn_stats_merge_kernel": 8, "bn_stats_merge_groups_kernel": 8}


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_rows_mma_instances_keep_registers_lds_and_occupancy(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in SOURCES]
    seen, bn_seen = dict.fromkeys(INSTANCES, 0), set()
    for src, proc in zip(SOURCES, procs):
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            # (anonymous namespace)::NAME[<[int, ]bool>]: _ZN12_GLOBAL__N_1<len>NAME [I [Li<pass>E] Lb<grouped>E E] E ...
            m = re.match(r"_ZN12_GLOBAL__N_1\d+((?:rows_bn_act|bn_stats_merge)\w*?_kernel)(?:I(?:Li(\d)E)?Lb(\d)EE|E)", b)
            if m:
                name = m.group(1)
                if m.group(3):
                    name += "<" + (m.group(2) + ", " if m.group(2) else "") + ("true" if m.group(3) == "1" else "false") + ">"
                assert field("ScratchSize [bytes/lane]") == 0, name
                assert field("VGPRs Spill") == 0, name
                assert field("Occupancy [waves/SIMD]") >= BN_WAVES[name], name
                bn_seen.add(name)
                continue
            # (anonymous namespace)::NAME<int, int[, bool]>: _ZN12_GLOBAL__N_1<len>NAME I Li<a>E Li<b>E [Lb<c>E] E ...
            m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)ILi(\d)ELi(\d)E(?:Lb(\d)E)?E", b)
            if not m or m.group(1) not in INSTANCES:
                continue
            kernel, n, mode = m.group(1), int(m.group(2)), int(m.group(3))
            name = f"{kernel}<{n}, {mode}" + (f", {m.group(4)}>" if m.group(4) else ">")
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
    assert bn_seen == set(BN_WAVES)
