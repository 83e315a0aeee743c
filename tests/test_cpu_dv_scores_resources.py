"""CPU-side check (no GPU needed): the d = 256 instances of the dV-from-scores kernel (csrc/attn_dv_scores.hip) compile for
gfx950 without scratch memory and without spilled vector registers, under 192 vector registers (the kernel declares the two-wave bound of 256: its tile images — 64 KB of dO^T planes, 32 KB of scores — leave no room for a second work-group on a
CU, so the four-wave bound of 128 registers would buy nothing) and inside the 160 KB of LDS of a CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGISTER_BOUND = 192          # the kernel is at 175 (dropout live) / 160: a regression shows long before the launch bound's 256


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_dv_scores_instances_fit_registers_and_lds(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    src = os.path.join(ROOT, "csn_amd", "csrc", "attn_dv_scores.hip")
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "dv.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if "csn_attn_dv_scores_kernel" not in name:
            continue
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        assert field("ScratchSize [bytes/lane]") == 0, name
        assert field("VGPRs Spill") == 0, name
        assert field("AGPRs") == 0, name                 # (the accumulators stay in the vector file: no moves around the products)
        assert field("VGPRs") <= REGISTER_BOUND, name
        assert field("Occupancy [waves/SIMD]") >= 2, name
        assert field("LDS Size [bytes/block]") <= 160 * 1024, name
        seen += 1
    assert seen == 2                                     # d = 256, dropout live / off
