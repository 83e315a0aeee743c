"""CPU-side check (no GPU needed): every instance of the fused LayerNorm-backward stream (csrc/wx_lnb.hip) compiles for gfx950
without scratch memory and without spilled vector registers, inside the 160 KB of LDS of a CU.  The kernel sits at 254-256
vector registers; a spill there hoists the commit's loads and costs the launch its pace (see csn_launch_wx_lnb)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_lnb_instance_fits_its_registers_and_lds(tmp_path):
    from csn_amd import _lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    src = os.path.join(ROOT, "csn_amd", "csrc", "wx_lnb.hip")
    res = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "wx_lnb.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if "csn_wx_lnb_kernel" not in name:
            continue
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        assert field("ScratchSize [bytes/lane]") == 0, name
        assert field("VGPRs Spill") == 0, name
        assert field("LDS Size [bytes/block]") <= 160 * 1024, name
        seen += 1
    assert seen == 4                                     # <DROP = true> x <RES> x <RED>
