"""CPU-side check (no GPU needed) of the one LDS tile image of the 64-query attention form (csn_amd/csrc/attn_tile_image.h): a
stand-alone host program (tests/tile_image_banks.cpp) includes the header, enumerates one wave's byte addresses for the
staging store, the transposing read and the row read — every wave, piece, k-step, channel group, read and both planes — and
counts per lane group the worst number of distinct addresses on one bank (stores on 32 banks in 8-lane groups; the
transposing read on 64 banks in 32-lane halves; the 16-byte row read on 64 banks in its four 16-lane groups).

DESIGN.md §4m states the image as conflict-free for all three: 1 / 1 / 1.  The program also checks what makes ONE image
correct: the three offset functions address the same byte for the same (row, key, plane), each access reaches every element of
the tile exactly once, and a lane's two score accumulators hold its 8 consecutive keys."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.skipif(_cxx() is None, reason="no host compiler")
def test_tile_image_is_conflict_free_and_one_image(tmp_path):
    exe = tmp_path / "tile_image_banks"
    res = subprocess.run([_cxx(), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "csn_amd", "csrc"),
                          os.path.join(ROOT, "tests", "tile_image_banks.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    print(out)
    words = out.split()
    got = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert got["mismatches"] == 0
    assert (got["store"], got["tr"], got["row"]) == (1, 1, 1)
