"""Time the MinkowskiNet head's fc_layer (csn_amd.minkowski_csn.BackboneFC: 1x1 convolution + BatchNorm + ReLU, training-mode
forward + backward) in math modes 0 and 1 beside the eager composition F.linear + F.batch_norm + relu on the same device.
HIP events around each iteration, median of ``--iters`` after ``--warmup``.  Prints one JSON line; ``--out`` also writes it.

    python scripts/bench_rows_fc.py --rows 32768 --c-in 480 --c-out 256 --out profiles/rows_fc_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--c-in", type=int, default=480)
    ap.add_argument("--c-out", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import functional as CF
    from csn_amd.minkowski_csn import BackboneFC
    torch.manual_seed(0)
    N, ci, co = a.rows, a.c_in, a.c_out
    m = BackboneFC(ci, co).cuda().train()
    x = torch.randn(N, ci, device="cuda", requires_grad=True)
    dy = torch.randn(N, co, device="cuda")
    params = [x] + list(m.parameters())

    def ours():
        for p in params:
            p.grad = None
        m(x).backward(dy)

    def eager():
        for p in params:
            p.grad = None
        bn = m[1]
        z = F.linear(x, m[0].weight, m[0].bias)
        F.relu(F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)).backward(dy)

    res = {"rows": N, "c_in": ci, "c_out": co, "warmup": a.warmup, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for mode in (0, 1):
        with CF.math_mode(mode):
            res[f"mode{mode}_fwd_bwd_ms"] = timed(ours, a.warmup, a.iters)
    res["eager_fwd_bwd_ms"] = timed(eager, a.warmup, a.iters)
    # bytes every implementation has to move at least once: forward reads x, writes z and y; backward reads dy, y, z (two passes),
    # dz three times (written, dx, dw), x once more, writes dx
    floats = N * ci * 3 + N * co * 12
    res["min_traffic_mb"] = floats * 4 / 1e6
    for mode in (0, 1):
        res[f"mode{mode}_gbps_of_min_traffic"] = floats * 4 / 1e9 / (res[f"mode{mode}_fwd_bwd_ms"] * 1e-3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
