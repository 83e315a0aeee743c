#!/usr/bin/env python3
"""Time the kernel-2 stride-2 convolutions (include/csn_hip.h section 21) and ``Res16UNet34C`` (csn_amd/minkowski_unet.py).
Development aid, not the headline bench.

  products   ``octant_conv_down`` / ``octant_conv_up``, forward and forward + backward (gradients to the rows and the weight), at
             ``--voxels`` (32768) fine voxels, 96 -> 96 and 256 -> 256, beside the eager composition a user has without them: per
             octant ``index_select``, ``matmul`` and ``index_add_`` (down) / ``index_copy_`` (up), through autograd.
  network    ``Res16UNet34C`` training forward + backward at the same voxels, ``fused=True`` beside ``fused=False``.
  shares     what the fused step spends outside the fused kernels, each timed alone on maps of the network's own sizes: the eight
             ATen BatchNorm + ReLU after the octant convolutions, and the ``cat_conv3d`` layers of the decoder blocks wider than
             256 columns (with their ATen BatchNorm).  Reported as milliseconds and as a share of the fused step.

Voxels: 8 synthetic ellipsoid shells (scripts/bench_sparse_conv.py).  Maps and pyramids are built once outside the timed window.
HIP events around each step; every variant is warmed up, then timed in ``--rounds`` alternating rounds of ``--iters`` steps in one
process: the figure is the median over the rounds of each round's median, ``spread`` its min and max over the rounds
(scripts/bench_hrnet.py).  Prints one JSON line.

    python scripts/bench_unet.py --out profiles/unet_bench.json
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_hrnet import compare  # noqa: E402
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def eager_octant(omap):
    """The two products as torch ops: (down(x, w), up(x, w)) over per-octant index lists built once."""
    order, seg = omap.order.long(), omap.seg.tolist()
    rows = [order[seg[k]:seg[k + 1]] for k in range(8)]
    par = [omap.parent.long()[r] for r in rows]

    def down(x, w):
        y = x.new_zeros(omap.n_coarse, w.shape[2])
        for k in range(8):
            if rows[k].numel():
                y.index_add_(0, par[k], x.index_select(0, rows[k]) @ w[k])
        return y

    def up(x, w):
        y = x.new_empty(omap.n_fine, w.shape[2])
        for k in range(8):
            if rows[k].numel():
                y.index_copy_(0, rows[k], x.index_select(0, par[k]) @ w[k])
        return y
    return down, up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mode", default="bf16x3", help="math mode: fp32 or bf16x3 (the library's default)")
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import Res16UNet34C, build_octant_map, build_unet_pyramid, octant_conv_down, octant_conv_up
    from csn_amd import functional as CF
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    n = coords.shape[0]
    res = {"voxels": int(n), "shapes": a.shapes, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "mode": a.mode,
           "device": torch.cuda.get_device_name(0)}

    with CF.math_mode(CF.mode_id(a.mode)):
        omap = build_octant_map(coords)
        res["octant_rows"] = {"fine": omap.n_fine, "coarse": omap.n_coarse, "segments": (omap.seg[1:] - omap.seg[:-1]).tolist()}
        e_down, e_up = eager_octant(omap)
        res["products"] = {}
        for c in (96, 256):
            w = (torch.randn(8, c, c, device="cuda") / (8 * c) ** 0.5).requires_grad_(True)
            for name, n_in, n_out, native, eager in (("down", omap.n_fine, omap.n_coarse, octant_conv_down, e_down),
                                                     ("up", omap.n_coarse, omap.n_fine, octant_conv_up, e_up)):
                x = torch.randn(n_in, c, device="cuda", requires_grad=True)
                dy = torch.randn(n_out, c, device="cuda")

                def fwd_of(f):
                    def step():
                        with torch.no_grad():
                            f()
                    return step

                def both_of(f):
                    def step():
                        x.grad = w.grad = None
                        f().backward(dy)
                    return step
                nat, eag = (lambda: native(x, w, None, omap)), (lambda: eager(x, w))
                r = compare({"native_fwd": fwd_of(nat), "eager_fwd": fwd_of(eag), "native_fwd_bwd": both_of(nat),
                             "eager_fwd_bwd": both_of(eag)}, a.warmup, 2 * a.iters, a.rounds)
                r["speedup_fwd"] = r["eager_fwd_ms"] / r["native_fwd_ms"]
                r["speedup_fwd_bwd"] = r["eager_fwd_bwd_ms"] / r["native_fwd_bwd_ms"]
                res["products"][f"{name}_{c}to{c}"] = r

        if not a.skip_network:
            pyr = build_unet_pyramid(coords)
            res["level_rows"] = [int(c.shape[0]) for c in pyr.coords]
            feats = torch.randn(n, 3, device="cuda")
            nets = {"fused": Res16UNet34C(3, 16, fused=True).cuda().train(), "unfused": Res16UNet34C(3, 16, fused=False).cuda().train()}
            nets["unfused"].load_state_dict(nets["fused"].state_dict())
            dy = torch.randn(n, 16, device="cuda")

            def step_of(net):
                def step():
                    for p in net.parameters():
                        p.grad = None
                    net((pyr, feats)).backward(dy)
                return step
            res["Res16UNet34C_train_fwd_bwd"] = compare({v: step_of(net) for v, net in nets.items()}, a.warmup, a.iters, a.rounds)
            fused_ms = res["Res16UNet34C_train_fwd_bwd"]["fused_ms"]

            # the shares: the same modules on maps of the network's sizes, alone
            net = nets["fused"]
            norms = [(getattr(net, f"bn{i}"), pyr.coords[i].shape[0]) for i in (1, 2, 3, 4)] + \
                    [(getattr(net, f"bntr{i}"), pyr.coords[7 - i].shape[0]) for i in (4, 5, 6, 7)]
            maps = [torch.randn(rows, m.num_features, device="cuda", requires_grad=True) for m, rows in norms]

            def bn_step():
                for (m, _), z in zip(norms, maps):
                    z.grad = m.weight.grad = m.bias.grad = None
                    F.relu(m(z)).sum().backward()
            wide = []
            for i in range(5, 9):
                blk = getattr(net, f"block{i}")[0]
                if blk.inplanes > 256:
                    level = 8 - i
                    rows = pyr.coords[level].shape[0]
                    up_c = getattr(net, f"bntr{i - 1}").num_features
                    parts = [torch.randn(rows, c, device="cuda", requires_grad=True) for c in (up_c, blk.inplanes - up_c)]
                    wide.append((blk, parts, pyr.s1[level], pyr.one[level]))

            def cat_step():
                for blk, parts, s1, one in wide:
                    for p in parts + list(blk.parameters()):
                        p.grad = None
                    y = F.relu(blk.norm1(blk.conv1(parts, s1))) + blk.downsample[1](blk.downsample[0](parts, one))
                    y.sum().backward()
            r = compare({"octant_norms": bn_step, "cat_conv_layers": cat_step}, a.warmup, a.iters, a.rounds)
            r["wide_blocks"] = [b.inplanes for b, *_ in wide]
            r["octant_norms_share_of_fused_step"] = r["octant_norms_ms"] / fused_ms
            r["cat_conv_layers_share_of_fused_step"] = r["cat_conv_layers_ms"] / fused_ms
            res["shares"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
