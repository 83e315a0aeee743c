"""CPU-side check (no GPU needed): the 64-query instance of the d = 256 bf16x3 attention backward (csrc/attn_bf16x3.hip, WG64)
compiles for gfx950 inside what two work-groups per CU allow: at most 256 vector registers at two waves per SIMD, at most 80 KB
of LDS per work-group (two groups in the 160 KB of a CU), and no more scratch or spilled registers than the eight-wave instance
it replaces, read from the same compile: the folded dQ <Bf16x3, 8, true, true, false, 2, true>.  (The forward's 64-query instance
is not built: DESIGN.md §4m "Two work-groups per CU".)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# template arguments behind the mode type: DT, BWD, KVP, RC, NOP, KV_SAME, WG64 (the itanium mangling of the instance names)
DQ_WG64, DQ_8W = "Li8ELb1ELb1ELb0ELi2ELb0ELb1E", "Li8ELb1ELb1ELb0ELi2ELb1ELb0E"


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    src = os.path.join(ROOT, "csn_amd", "csrc", "attn_bf16x3.hip")
    out = tmp_path_factory.mktemp("wg64") / "attn.o"
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(out)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    table = {}
    for b in re.split(r"remark: Function Name: ", res.stderr)[1:]:
        name = b.split()[0]
        if "csn_attn_bf16x3_kernel" in name and "Bf16x3E" in name:
            table[name] = {key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
                           for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs", "Occupancy [waves/SIMD]",
                                       "LDS Size [bytes/block]")}
    return table


def _one(table, args):
    hits = [v for n, v in table.items() if args in n]
    assert len(hits) == 1, (args, sorted(table))
    return hits[0]


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
@pytest.mark.parametrize("new,old", [(DQ_WG64, DQ_8W)], ids=["dq"])
def test_wg64_instance_fits_two_groups_per_cu(usage, new, old):
    n, o = _one(usage, new), _one(usage, old)
    print(new, n, "replaces", o)
    assert n["VGPRs"] <= 256
    assert n["Occupancy [waves/SIMD]"] == 2
    assert n["LDS Size [bytes/block]"] <= 80 * 1024
    assert n["ScratchSize [bytes/lane]"] <= o["ScratchSize [bytes/lane]"]
    assert n["VGPRs Spill"] <= o["VGPRs Spill"]
