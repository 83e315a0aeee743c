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

``--infer`` times the eval variants instead and nothing else: the 3S backbone forward in eval mode under ``torch.no_grad()`` with
``tuning.eval_epilogue`` off (``two_launch``: ``sparse_conv3d`` + ``bn_act`` per convolution, then ``torch.cat``) against on
(``one_launch``: include/csn_hip.h section 19, the result written in place), in math modes fp32 and bf16x3, the same rounds.
``counted_bytes`` is the traffic of the output maps alone that the two graphs differ in (``infer_bytes``); the gathers and the
weights are the same reads in both.

    python scripts/bench_hrnet.py --infer --out profiles/hrnet_infer_bench.json
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


def infer_bytes(num_stages, D, init_dim, rows):
    """Bytes of the maps written and read back between a convolution's accumulators and the next convolution's gather, per forward:
    (two_launch, one_launch).  With e = 4 n c for an (n, c) map — two launches: a convolution writes z (e), ``bn_act`` reads every
    z of its sum and the residual or own map and writes y; ``torch.cat`` reads and writes the result once.  One launch: every
    launch writes y and reads its residual (the own map, or the running sum)."""
    two = one = 0
    e = lambda level, c: 4 * rows[level] * c

    def conv(level, c, paths=1, res=0):
        nonlocal two, one
        two += (2 * paths + res + 1) * e(level, c)                          # z written and read per path, r read, y written
        one += (2 * paths - 1 + res) * e(level, c)                          # y written per launch, r / the running sum read
    conv(0, init_dim)
    conv(0, D)
    for i in range(num_stages):
        for j in range(i + 1):
            for _ in range(3):
                conv(j, D * 2 ** j)
                conv(j, D * 2 ** j, res=1)
        if i == num_stages - 1:
            break
        depth = i + 1
        for k in range(depth + 1):
            sources = [j for j in range(depth) if j != k]
            for j in sources:
                for s in range(abs(k - j) - 1):                             # the inner steps of a multi-step path
                    level = j + s + 1 if k > j else j - s - 1
                    conv(level, D * 2 ** level)
            if sources:
                conv(k, D * 2 ** k, paths=len(sources), res=int(k < depth))
    for i in range(1, num_stages):
        for s in range(i):
            conv(i - s - 1, D * 2 ** i)
    two += 2 * 4 * rows[0] * (init_dim + sum(D * 2 ** s for s in range(num_stages)))      # torch.cat: read + write
    return two, one


def infer(a):
    import csn_amd
    csn_amd.build()
    from csn_amd import HRNetBackbone, build_pyramid
    from csn_amd import functional as CF
    from csn_amd import tuning
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_pyramid(coords, 3)
    n = coords.shape[0]
    rows = [int(c.shape[0]) for c in pyr.coords]
    two, one = infer_bytes(3, 64, 32, rows)
    res = {"voxels": int(n), "level_rows": rows, "shapes": a.shapes, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "what": "HRNetBackbone 3S forward, eval, no_grad",
           "counted_bytes": {"two_launch": two, "one_launch": one}}
    feats = torch.randn(n, 3, device="cuda")
    net = HRNetBackbone(3, 3, 2).cuda().eval()

    def step_of(mode, on):
        def step():
            with torch.no_grad(), CF.math_mode(mode), tuning.override(eval_epilogue=on):
                net(feats, pyr)
        return step
    for mode in ("fp32", "bf16x3"):
        r = compare({"two_launch": step_of(mode, False), "one_launch": step_of(mode, True)}, a.warmup, a.iters, a.rounds)
        gap = r["two_launch_ms"] - r["one_launch_ms"]
        noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in ("two_launch", "one_launch"))
        r["speedup"] = r["two_launch_ms"] / r["one_launch_ms"]
        r["one_launch_is_faster"] = bool(gap > noise and r["one_launch_spread_ms"][1] < r["two_launch_spread_ms"][0])
        res[f"backbone_3S_eval_fwd_{mode}"] = r
    return res


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
    ap.add_argument("--infer", action="store_true", help="time the eval variants (eval_epilogue off against on, fp32 and bf16x3) instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.infer:
        line = json.dumps(infer(a))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
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
