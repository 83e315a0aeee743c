"""Time one sparse 3D convolution (csn_amd.minkowski_conv.sparse_conv3d), forward and backward, at the HRNet3S geometry beside the
eager composition on the same device in the same process: per kernel offset ``index_select`` + ``matmul`` + ``index_add_`` (and
its autograd backward), with the per-offset row lists built beforehand as the kernel map is.

Voxels: ``--voxels`` (32768) from 8 synthetic surface-like shapes — ellipsoid shells voxelised, so neighbour counts resemble real
shapes, not a filled cube.  Layers: 64 -> 64 on the voxels, 128 -> 128 on their stride-2 set, 256 -> 256 on the stride-4 set (k = 3),
and the stem 3 -> 32 at k = 5 (the wrapper pads its rows to 32 channels; the padding is inside the timed call).

HIP events around each call; every variant is warmed up, then timed in ``--rounds`` alternating rounds of ``--iters`` calls: the
figure is the median over the rounds of each round's median, ``spread`` its min and max over the rounds.  FLOP counts only the
matrix products of existing (offset, row) pairs: forward 2 P c_in c_out, backward twice that (dx and dw).  ``min_mb`` is what any
implementation has to move once: forward x, table, W, y; backward dy, x, both tables, W, dx, dW — a lower bound computed from the
shapes, not measured traffic.  The forward call is one launch; the backward call is the sum of its launches (dx, dW, the slab
sum, the two dbias kernels when there is a bias).  Per-launch times and memory-side bytes come from profiler passes over
``--layers NAME --variants mode1`` (profiles/sparse_conv_launches.txt).  ``mode2`` (bf16 forward + backward) and ``mode3`` (fp16
forward, bf16 backward) are the single-product row products: both run with ``tuning.rows_single_product`` on.  Prints one JSON line.

    python scripts/bench_sparse_conv.py --out profiles/sparse_conv_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shell_shapes(n_shapes, per_shape):
    """[b, x, y, z] int64 rows: per shape the first ``per_shape`` voxels (sorted) of the thinnest ellipsoid shell that holds as many."""
    rows = []
    for s in range(n_shapes):
        ax = torch.tensor([1.0, 0.8 + 0.05 * s, 1.2 - 0.04 * s])
        r = (per_shape / 12.6) ** 0.5 * 0.8
        while True:
            side = int(r * 1.3) + 2
            a = torch.arange(-side, side + 1)
            p = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), dim=-1).reshape(-1, 3)
            d = ((p.double() / ax.double()) ** 2).sum(1).sqrt()
            shell = p[(d - r).abs() < 0.5]
            if shell.shape[0] >= per_shape:
                break
            r += 0.25
        rows.append(torch.cat([torch.full((per_shape, 1), s), shell[:per_shape]], dim=1))
    return torch.cat(rows)


def timed(prepare, fn, iters):
    ms = []
    for _ in range(iters):
        state = prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(state)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", default="", help="comma-separated substrings of the layer names to run (default: all)")
    ap.add_argument("--variants", default="mode0,mode1,eager",
                    help="which of mode0, mode1, mode2, mode3, eager to run (a profiler pass wants one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import functional as CF
    from csn_amd import tuning
    from csn_amd.minkowski_conv import build_kernel_map, sparse_conv3d
    torch.manual_seed(0)
    c1 = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    down1 = build_kernel_map(c1, 3, stride=2, tensor_stride=1)
    down2 = build_kernel_map(down1.out_coords, 3, stride=2, tensor_stride=2)
    layers = [("64to64_k3", build_kernel_map(c1, 3, tensor_stride=1), 64, 64),
              ("128to128_k3_stride2_set", build_kernel_map(down1.out_coords, 3, tensor_stride=2), 128, 128),
              ("256to256_k3_stride4_set", build_kernel_map(down2.out_coords, 3, tensor_stride=4), 256, 256),
              ("stem_3to32_k5", build_kernel_map(c1, 5, tensor_stride=1), 3, 32)]
    res = {"voxels": int(c1.shape[0]), "shapes": a.shapes, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "layers": {}}
    picked = [s for s in a.layers.split(",") if s]
    for name, m, ci, co in layers:
        if picked and not any(s in name for s in picked):
            continue
        KV, n = m.KV, m.n_in
        x = torch.randn(n, ci, device="cuda", requires_grad=True)
        w = (torch.randn(KV, ci, co, device="cuda") / (KV * ci) ** 0.5).requires_grad_(True)
        dy = torch.randn(n, co, device="cuda")
        lists = [((m.fwd[k] >= 0).nonzero().squeeze(1), m.fwd[k][m.fwd[k] >= 0].long()) for k in range(KV)]
        pairs = int(sum(j.numel() for j, _ in lists))

        def ours(_=None):
            return sparse_conv3d(x, w, None, m)

        def eager(_=None):
            y = torch.zeros(n, co, device="cuda")
            for k, (j, i) in enumerate(lists):
                if j.numel():
                    y = y.index_add(0, j, x.index_select(0, i) @ w[k])
            return y

        def back(y):
            x.grad = w.grad = None
            y.backward(dy)

        variants = {"mode0": (0, ours), "mode1": (1, ours), "mode2": (2, ours), "mode3": (3, ours), "eager": (None, eager)}
        variants = {v: variants[v] for v in a.variants.split(",")}
        cip = -(-ci // 32) * 32
        mb_f = (n * cip + KV * n + KV * cip * co + n * co) * 4 / 1e6
        mb_b = (n * co + n * cip + 2 * KV * n + 2 * KV * cip * co + n * cip) * 4 / 1e6
        out = {"rows": n, "pairs": pairs, "mean_neighbours": pairs / n, "fwd_gflop": 2 * pairs * ci * co / 1e9,
               "bwd_gflop": 4 * pairs * ci * co / 1e9, "fwd_min_mb": mb_f, "bwd_min_mb": mb_b}
        samples = {(v, p): [] for v in variants for p in ("fwd", "bwd")}
        for rnd in range(a.rounds + 1):                                          # round 0 is the warm-up
            it = a.warmup if rnd == 0 else a.iters
            for v, (mode, fn) in variants.items():
                with CF.math_mode(mode), tuning.override(rows_single_product=v in ("mode2", "mode3")):
                    tf = timed(lambda: None, fn, it)
                    tb = timed(fn, back, it)
                if rnd:
                    samples[(v, "fwd")].append(tf)
                    samples[(v, "bwd")].append(tb)
        for (v, p), s in samples.items():
            t = statistics.median(s)
            out[f"{v}_{p}_ms"] = t
            out[f"{v}_{p}_spread_ms"] = [min(s), max(s)]
            if v != "eager":
                out[f"{v}_{p}_tflops"] = out[f"{p}_gflop"] / t
                out[f"{v}_{p}_gbps_of_min_traffic"] = out[f"{p}_min_mb"] / t
        res["layers"][name] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
