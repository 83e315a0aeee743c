"""Time the K + 1 backbone passes of a CSN training step as SEPARATE passes (one ``HRNetBackbone`` forward + backward per batch: the
path ``HRNetSimCSN.forward`` takes by default) against ONE grouped pass on the merged pyramid (``merge_batches`` + BatchNorm over row
groups, include/csn_hip.h section 20: what ``tuning.grouped_passes`` selects) on the same device in the same process.

Workload: the 3S backbone, training forward + backward, ``--groups`` (4) batches of ``--shapes`` (8) synthetic ellipsoid shells at
``--voxels`` (32768) voxels each (scripts/bench_sparse_conv.py), in math modes bf16x3 and fp32.  The pyramids are built once outside
the timed window, as a training loop would per batch.  A step of either variant starts from cleared gradients and ends with the
weight gradients of all batches summed (autograd adds the separate passes'; the grouped pass forms one sum).  HIP events around
each step; both variants are warmed up, then timed in ``--rounds`` alternating rounds of ``--iters`` steps: the figure is the median
over the rounds of each round's median, ``spread`` its min and max over the rounds.  ``grouped_is_faster`` is true only when the
grouped median lies below the separate one by more than both spreads.  ``--only separate|grouped`` runs one variant in one mode
(``--mode``) and prints no comparison: what a profiler pass wants, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o grouped -- python scripts/bench_hrnet_groups.py --only grouped --rounds 1

Prints one JSON line.

    python scripts/bench_hrnet_groups.py --out profiles/hrnet_groups_bench.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_hrnet import compare  # noqa: E402
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768, help="voxels per batch")
    ap.add_argument("--shapes", type=int, default=8, help="shapes per batch")
    ap.add_argument("--groups", type=int, default=4, help="batches of a step (K + 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="separate or grouped: run that variant alone, in --mode")
    ap.add_argument("--mode", default="bf16x3", help="math mode of an --only run: fp32 or bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import HRNetBackbone, build_pyramid, merge_batches
    from csn_amd import functional as CF
    torch.manual_seed(0)
    # every batch the same shells moved by its own offset: the same row counts per level, other coordinates
    base = shell_shapes(a.shapes, a.voxels // a.shapes)
    coords = [(base + torch.tensor([0, 3 * g, -2 * g, g])).cuda() for g in range(a.groups)]
    pyrs = [build_pyramid(c, 3) for c in coords]
    gp = merge_batches([(c, None) for c in coords], 3, n_shapes=[a.shapes] * a.groups)
    n = [int(c.shape[0]) for c in coords]
    feats = [torch.randn(k, 3, device="cuda") for k in n]
    net = HRNetBackbone(3, 3, 2).cuda().train()
    dys = [torch.randn(k, net.out_channels, device="cuda") for k in n]
    feats_all, dy_all = torch.cat(feats), torch.cat(dys)
    res = {"voxels_per_batch": n, "groups": a.groups, "shapes": a.shapes, "level_rows_per_batch": [int(c.shape[0]) for c in pyrs[0].coords],
           "level_rows_merged": [int(c.shape[0]) for c in gp.coords], "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "what": "HRNetBackbone 3S, training forward + backward of all batches"}

    def step_of(variant, mode):
        def step():
            for p in net.parameters():
                p.grad = None
            with CF.math_mode(mode):
                if variant == "grouped":
                    net(feats_all, gp).backward(dy_all)
                else:
                    for f, p, d in zip(feats, pyrs, dys):
                        net(f, p).backward(d)
        return step
    if a.only:
        r = compare({a.only: step_of(a.only, a.mode)}, a.warmup, a.iters, a.rounds)
        res[f"backbone_3S_train_fwd_bwd_{a.mode}"] = r
    else:
        for mode in ("bf16x3", "fp32"):
            r = compare({"separate": step_of("separate", mode), "grouped": step_of("grouped", mode)}, a.warmup, a.iters, a.rounds)
            gap = r["separate_ms"] - r["grouped_ms"]
            noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in ("separate", "grouped"))
            r["speedup"] = r["separate_ms"] / r["grouped_ms"]
            r["grouped_is_faster"] = bool(gap > noise and r["grouped_spread_ms"][1] < r["separate_spread_ms"][0])
            res[f"backbone_3S_train_fwd_bwd_{mode}"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
