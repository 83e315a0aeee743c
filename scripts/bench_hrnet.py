"""Time the HRNet3S backbone (csn_amd.minkowski_hrnet.HRNetBackbone), training forward + backward, with the fused BatchNorm kernels
(``fused=True``: include/csn_hip.h section 15) beside the same graph on ``sparse_conv3d`` + ATen batch norm / add / ReLU
(``fused=False``) on the same device in the same process; and one ``HRBasicBlock`` beside ``SparseBasicBlock`` at 64 / 128 / 256
channels on the voxel set of the branch that has that width.

Voxels: ``--voxels`` (32768) from 8 synthetic ellipsoid shells (scripts/bench_sparse_conv.py).  The pyramid is built once outside
the timed window, as a training loop would per batch.  HIP events around each forward + backward; every variant is warmed up, then
timed in ``--rounds`` alternating rounds of ``--iters`` steps: the figure is the median over the rounds of each round's median,
``spread`` its min and max over the rounds.  ``fused_is_faster`` is true only when the fused median lies below the unfused one by more
than both spreads.  ``--only fused|unfused`` runs one variant (a profiler pass wants one).  ``--variants`` names the variants
outright and adds ``mode2`` (bf16 forward + backward) and ``mode3`` (fp16 forward, bf16 backward): the fused network on the
single-product row products (``tuning.rows_single_product`` on), whatever ``--mode`` says; ``--mode bf16`` / ``fp16`` runs ``fused`` and
``unfused`` so too.  Prints one JSON line.

    python scripts/bench_hrnet.py --out profiles/hrnet_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def timed(step, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def compare(variants, warmup, iters, rounds):
    """variants: name -> step().  Alternating rounds (round 0 is the warm-up); medians of the rounds' medians and their spread."""
    samples = {v: [] for v in variants}
    for rnd in range(rounds + 1):
        for v, step in variants.items():
            t = timed(step, warmup if rnd == 0 else iters)
            if rnd:
                samples[v].append(t)
    out = {}
    for v, s in samples.items():
        out[f"{v}_ms"] = statistics.median(s)
        out[f"{v}_spread_ms"] = [min(s), max(s)]
    if "unfused_ms" in out and "fused_ms" in out:
        gap = out["unfused_ms"] - out["fused_ms"]
        noise = max(out["fused_spread_ms"][1] - out["fused_spread_ms"][0], out["unfused_spread_ms"][1] - out["unfused_spread_ms"][0])
        out["speedup"] = out["unfused_ms"] / out["fused_ms"]
        out["fused_is_faster"] = bool(gap > noise and out["fused_spread_ms"][1] < out["unfused_spread_ms"][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mode", default="bf16x3", help="math mode of fused / unfused: fp32, bf16x3 (the library's default), bf16 or fp16")
    ap.add_argument("--only", default="", help="fused or unfused: run that variant alone")
    ap.add_argument("--variants", default="", help="comma-separated: fused, unfused, mode2, mode3 (default: fused,unfused)")
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import HRBasicBlock, HRNetBackbone, SparseBasicBlock, build_pyramid
    from csn_amd import functional as CF
    from csn_amd import tuning
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_pyramid(coords, 3)
    n = coords.shape[0]
    res = {"voxels": int(n), "level_rows": [int(c.shape[0]) for c in pyr.coords], "shapes": a.shapes, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "mode": a.mode, "device": torch.cuda.get_device_name(0)}
    feats = torch.randn(n, 3, device="cuda")
    want = [v for v in a.variants.split(",") if v] or [v for v in ("fused", "unfused") if not a.only or v == a.only]
    # a variant's math mode, and whether it runs the single-product row products
    arith = {v: {"mode2": (2, True), "mode3": (3, True)}.get(v, (CF.mode_id(a.mode), CF.mode_id(a.mode) >= 2)) for v in want}

    with CF.math_mode(CF.mode_id(a.mode)), tuning.override(rows_single_product=CF.mode_id(a.mode) >= 2):
        nets = {v: HRNetBackbone(3, 3, 2, fused=(v != "unfused")).cuda().train() for v in want}
        for v in want[1:]:
            nets[v].load_state_dict(nets[want[0]].state_dict())
        dy = torch.randn(n, nets[want[0]].out_channels, device="cuda")

        def step_of(v):
            net, (mode, single) = nets[v], arith[v]

            def step():
                for p in net.parameters():
                    p.grad = None
                with CF.math_mode(mode), tuning.override(rows_single_product=single):
                    net(feats, pyr).backward(dy)
            return step
        res["backbone_3S_train_fwd_bwd"] = compare({v: step_of(v) for v in want}, a.warmup, a.iters, a.rounds)
        del nets
        want = [v for v in want if v in ("fused", "unfused")]
        if not a.skip_blocks and want:
            res["blocks_train_fwd_bwd"] = {}
            for level, c in enumerate((64, 128, 256)):
                kmap, rows = pyr.s1[level], pyr.coords[level].shape[0]
                x = torch.randn(rows, c, device="cuda", requires_grad=True)
                dyb = torch.randn(rows, c, device="cuda")
                blocks = {"fused": HRBasicBlock(c, c).cuda().train(), "unfused": SparseBasicBlock(c, c).cuda().train()}
                blocks["unfused"].load_state_dict(blocks["fused"].state_dict())

                def bstep_of(blk):
                    def step():
                        x.grad = None
                        for p in blk.parameters():
                            p.grad = None
                        blk(x, kmap).backward(dyb)
                    return step
                r = compare({v: bstep_of(blocks[v]) for v in want}, a.warmup, 2 * a.iters, a.rounds)
                r["rows"] = int(rows)
                res["blocks_train_fwd_bwd"][f"{c}_wide"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
