"""CPU-side checks of the fused U-Net tail (include/csn_hip.h sections 26 and 27; ``tuning.unet_fused_tail``), no GPU needed: the
header, the exports and the Python surface carry the new names at ABI version 17; the switch defaults to False; the host-side
argument checks answer without a device; a numpy restatement of the count-aware Chan merge (rows_mma.h ``chan_walk_counts`` + the
pairwise tree of octant_conv_stats.hip) equals the direct biased / unbiased variance to 1e-12 on the tile counts of
tests/test_gpu_octant_stats.py's hand-made set — 0, 1, 31, 32 rows, short tiles in the middle of the list; the float64 reference of
tests/test_gpu_unet_fused_tail.py's cases has at most 0.1 % of its pre-activations within 1e-4 of zero; every kernel of the two new
translation units compiles for gfx950 without scratch or spilled registers; and the ``octant_rows_kernel`` / ``octant_rows_bn_kernel``
instances keep the vector registers and the occupancy they had before the body gained its third epilogue."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csn_octant_stats_workspace_bytes", "csn_octant_down_stats_fwd_f32", "csn_octant_up_stats_fwd_f32",
       "csn_sparse_conv_cat_stats_workspace_bytes", "csn_sparse_conv_cat_stats_fwd_f32")
E_ARG, E_ALIGN, E_PTR, E_DIM, E_WORKSPACE = -1, -2, -3, -5, -6


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


def test_header_exports_and_python_surface_carry_the_new_names(L):
    import csn_amd
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NEW:
        assert re.search(r"CSN_API (int|long long) " + name + r"\(", header), name
        assert name in L.EXPORTS and hasattr(L.lib(), name), name
    assert "typedef struct CsnCatParts" in header and "#define CSN_ABI_VERSION 17" in header
    assert L.lib().csn_version() == 17
    assert "sparse_conv_cat.hip" in L.SOURCES and "octant_conv_stats.hip" in L.SOURCES
    assert callable(csn_amd.octant_conv_stats) and callable(csn_amd.cat_conv_stats)
    assert ctypes.sizeof(L.CatParts) == 4 * 8 + 4 * 8 + 4 * 4


def test_the_switch_defaults_to_off():
    from csn_amd import tuning
    assert tuning.Tuning().unet_fused_tail is False and tuning.current().unet_fused_tail is False
    with tuning.override(unet_fused_tail=True):
        assert tuning.current().unet_fused_tail is True
    assert tuning.current().unet_fused_tail is False


def test_host_side_checks_answer_without_a_device(L):
    lib = L.lib()
    # workspace sizes: 0 for arguments the entry points refuse; up holds (ceil(n / 128) + 7) * 4 tiles of (mean, M2) and a count
    assert lib.csn_octant_stats_workspace_bytes(0, 5, 64, 1) == 0 and lib.csn_octant_stats_workspace_bytes(100, 20, 48, 1) == 0
    up = lib.csn_octant_stats_workspace_bytes(1000, 200, 64, 1)
    assert up >= (8 + 7) * 4 * (2 * 64 * 4 + 4)
    assert lib.csn_octant_stats_workspace_bytes(1000, 200, 64, 0) == lib.csn_sparse_conv_stats_workspace_bytes(200, 64)
    assert lib.csn_sparse_conv_cat_stats_workspace_bytes(200, 64) == lib.csn_sparse_conv_stats_workspace_bytes(200, 64)
    p = 4096                                                               # an aligned address that is never followed
    down = lambda **k: lib.csn_octant_down_stats_fwd_f32(k.get("x", p), k.get("ld_x", 64), k.get("n_fine", 100), p, k.get("n_coarse", 20),
                                                         k.get("c_in", 64), k.get("c_out", 64), p, k.get("z", p), k.get("ld_z", 64), p, p,
                                                         None, None, 1e-5, 0.1, p, k.get("ws", 1 << 30), None)
    upf = lambda **k: lib.csn_octant_up_stats_fwd_f32(k.get("x", p), k.get("ld_x", 64), k.get("n_coarse", 20), p, p, k.get("seg", p),
                                                      k.get("n_fine", 100), k.get("c_in", 64), k.get("c_out", 64), p, k.get("z", p),
                                                      k.get("ld_z", 64), p, p, None, None, 1e-5, 0.1, p, k.get("ws", 1 << 30), None)
    for f in (down, upf):
        assert f(x=None) == E_ARG and f(z=None) == E_ARG
        assert f(c_out=48) == E_DIM and f(c_in=288) == E_DIM
        assert f(ld_z=32) == E_ARG and f(ld_z=66) == E_ALIGN and f(ld_x=70) == E_ALIGN
        assert f(ws=16) == E_WORKSPACE
        assert f(z=p + 4) == E_PTR
    assert down(n_coarse=1) == E_ARG and upf(n_fine=1, n_coarse=1) == E_ARG    # a one-row BatchNorm batch
    assert upf(seg=p + 2) == E_PTR
    cp = L.CatParts()
    for m, c in enumerate((256, 32)):
        cp.x[m], cp.ld_x[m], cp.c_in[m] = p, c, c
    cat = lambda parts=cp, n_parts=2, **k: lib.csn_sparse_conv_cat_stats_fwd_f32(
        ctypes.byref(parts) if parts is not None else None, n_parts, 100, p, k.get("n_out", 100), k.get("kv", 27), k.get("c_out", 64), p, p,
        k.get("ld_z", 64), p, p, None, None, 1e-5, 0.1, p, k.get("ws", 1 << 30), None)
    assert cat(parts=None) == E_ARG and cat(n_parts=0) == E_ARG and cat(n_parts=5) == E_ARG
    assert cat(n_parts=3) == E_ARG                                         # the third part's pointer is NULL
    assert cat(kv=125) == E_DIM and cat(kv=8) == E_DIM and cat(c_out=300) == E_DIM
    assert cat(ld_z=66) == E_ALIGN and cat(ws=16) == E_WORKSPACE and cat(n_out=1) == E_ARG
    bad = L.CatParts()
    bad.x[0], bad.ld_x[0], bad.c_in[0] = p, 48, 48
    bad.x[1], bad.ld_x[1], bad.c_in[1] = p, 32, 32
    assert cat(parts=bad) == E_DIM
    bad.ld_x[0], bad.c_in[0] = 32, 64
    assert cat(parts=bad) == E_ARG                                         # a pitch below the part's width


def _merge(counts, means, m2s, segments=64):
    """The merge of octant_conv_stats.hip in numpy float64: ``segments`` runs of the tile list merged in tile order with each tile's
    own count (an empty tile is skipped), then the runs merged pairwise, neighbours first, the lower tiles on the left."""
    def chan(a, b):
        (n, mu, m2), (nb, mb, qb) = a, b
        if nb <= 0:
            return a
        nn, d = n + nb, mb - mu
        return nn, mu + d * (nb / nn), m2 + qb + d * d * (n * nb / nn)
    per = (len(counts) + segments - 1) // segments
    runs = []
    for s in range(segments):
        acc = (0.0, 0.0, 0.0)
        for t in range(min(len(counts), s * per), min(len(counts), s * per + per)):
            if counts[t] > 0:
                acc = chan(acc, (float(counts[t]), means[t], m2s[t]))
        runs.append(acc)
    stride = 1
    while stride < segments:
        for s in range(0, segments, 2 * stride):
            runs[s] = chan(runs[s], runs[s + stride])
        stride *= 2
    return runs[0]


def test_count_aware_chan_merge_equals_the_direct_variance():
    """The wave tiles of the hand-made set of tests/test_gpu_octant_stats.py (octants of 1, 2, 31, 32, 33, 0, 64, 65 rows cut into
    128-entry tiles of four 32-row waves, then seven empty row groups) and two lists with short tiles in the middle."""
    tiles_of = lambda segs: [max(0, min(32, n - 32 * w)) for n in segs for w in range(4)] if segs else []
    hand = tiles_of([1, 2, 31, 32, 33, 64, 65]) + [0] * (4 * 4)
    assert {0, 1, 31, 32} <= set(hand) and hand.index(1) < hand.index(32)
    rng = np.random.default_rng(3)
    for counts in (hand, [32, 0, 5, 32, 32, 1, 0, 0, 31, 32], [0, 0, 2], [32] * 70 + [7] + [32] * 70):
        rows = [rng.normal(3.0, 2.0, size=c) for c in counts]
        means = [float(r.mean()) if len(r) else 0.0 for r in rows]
        m2s = [float(((r - r.mean()) ** 2).sum()) if len(r) else 0.0 for r in rows]
        n, mu, m2 = _merge(counts, means, m2s)
        every = np.concatenate(rows)
        assert n == len(every)
        assert abs(mu - every.mean()) < 1e-12
        assert abs(m2 / n - every.var()) < 1e-12 and abs(m2 / (n - 1) - every.var(ddof=1)) < 1e-12


def test_reference_pre_activations_keep_their_distance_from_zero():
    """For exactly the cases of tests/test_gpu_unet_fused_tail.py: at most 0.1 % of the float64 pre-activations lie within 1e-4 of
    zero, over the network and in every single map."""
    from tests.test_gpu_unet import reference
    from tests.test_gpu_unet_fused_tail import N, NETS
    for net in NETS:
        _, pre, _ = reference(net, N, True)
        near = {k: (v.abs() < 1e-4).double().mean().item() for k, v in pre.items()}
        total = sum((v.abs() < 1e-4).sum().item() for v in pre.values()) / sum(v.numel() for v in pre.values())
        print(f"[unet tail] {net}: {total:.1e} of all pre-activations within 1e-4 of zero, at most {max(near.values()):.1e} in one map")
        assert total <= 1e-3 and max(near.values()) <= 1e-3, (net, total, max(near, key=near.get))


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


# VGPRs and waves per SIMD of the instances before the body gained its third epilogue: octant_rows_kernel<NB, MODE, B_KN> (the same
# for both B_KN but where noted) and octant_rows_bn_kernel<NB, MODE>
ROWS_BEFORE = {(1, 0): (54, 7), (1, 1): (65, 5), (2, 0): (66, 4), (2, 1): (75, 4), (3, 0): (70, 4), (3, 1): (80, 4), (4, 0): (90, 3),
               (4, 1): (87, 3)}
ROWS_BEFORE_B_NK = {(2, 1): (73, 4), (3, 0): (68, 4)}                       # the dx instances (B_KN false) that differ


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_new_kernels_have_no_scratch_and_the_old_instances_keep_their_registers(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    sources = ["octant_conv_stats.hip", "sparse_conv_cat.hip", "octant_conv.hip"]
    procs = [subprocess.Popen([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", s),
                               "-o", str(tmp_path / (s + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in sources]
    seen = {s: {} for s in sources}
    for s, proc in zip(sources, procs):
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        for b in re.split(r"Function Name: ", err)[1:]:
            field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
            seen[s][b.split()[0]] = {"scratch": field("ScratchSize [bytes/lane]"), "spill": field("VGPRs Spill"), "sspill": field("SGPRs Spill"),
                                     "vgprs": field("VGPRs"), "waves": field("Occupancy [waves/SIMD]")}
    new = {**seen["octant_conv_stats.hip"], **seen["sparse_conv_cat.hip"]}
    stats = [k for k in new if "octant_rows_stats_kernel" in k]
    acc = [k for k in new if "sconv_gemm_acc_kernel" in k]
    assert len(stats) == 8 and len(acc) == 16 and any("octant_stats_merge_kernel" in k for k in new)
    for k, r in new.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (k, r)
    old = seen["octant_conv.hip"]
    found = 0
    for k, r in old.items():
        m = re.match(r"_ZN12_GLOBAL__N_1\d+octant_rows_kernelILi(\d)ELi(\d)ELb(\d)EE", k)
        mb = re.match(r"_ZN12_GLOBAL__N_1\d+octant_rows_bn_kernelILi(\d)ELi(\d)EE", k)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            want = ROWS_BEFORE_B_NK.get(key, ROWS_BEFORE[key]) if m.group(3) == "0" else ROWS_BEFORE[key]
        elif mb:
            want = ROWS_BEFORE[(int(mb.group(1)), int(mb.group(2)))]
        else:
            continue
        found += 1
        assert (r["vgprs"], r["waves"]) == want and r["scratch"] == 0 and r["spill"] == 0, (k, r, want)
    assert found == 24
