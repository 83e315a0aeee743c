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

``--infer`` times the eval variants instead and nothing else: the forward of ``Res16UNet34C`` and of ``Res16UNet14`` (every decoder
block wider than 256 columns) in eval mode under ``torch.no_grad()`` with ``tuning.eval_epilogue`` off (``training_graph``: what
the networks ran before the switch reached them) against on (``one_launch``: ``Res16UNetBase._forward_infer``), in math modes fp32
and bf16x3, the same rounds in one process.  ``counted_bytes`` is the traffic of the maps between a convolution's accumulators and
the next gather (``infer_bytes``; the gathers and the weights are the same reads in both graphs), ``library_calls`` the C-ABI calls
of one forward.

In math modes bf16 and fp16 ``--infer`` times three routes of the one-launch graph, all with ``eval_epilogue + rows_single_product``
(``eval_fwd_bf16`` / ``eval_fwd_fp16``): ``fp32_maps`` as it stands (sections 19 and 23: the octant products bf16x3),
``octant16`` with ``octant_single_product`` (section 25 on fp32 maps) and ``maps16`` with ``unet_maps16`` (sections 24 and 25, every
stored map 16-bit).  ``counted_bytes_16`` counts, on the launches themselves, the bytes each route gathers ((valid table entries,
or fine rows) x c_in x element size), writes (the output maps) and reads as residuals, as scripts/bench_hrnet_maps16.py does.

    python scripts/bench_unet.py --infer --rounds 5 --out profiles/unet_infer_bench.json

``--train`` times the training step and nothing else: forward + backward of ``Res16UNet34C`` and ``Res16UNet14`` in math modes
bf16x3 and fp32, three columns in the same alternating rounds — ``fused=False``, ``fused`` and ``fused`` under
``tuning.unet_fused_tail`` (sections 26 and 27: no ATen normalisation left in the step).  The plain run carries the same third
column for ``Res16UNet34C`` in ``--mode``.

    python scripts/bench_unet.py --train --rounds 5 --iters 20 --out profiles/unet_fused_tail_bench.json
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


def infer_bytes(net, rows):
    """Bytes of the maps written and read back between a convolution's accumulators and the next convolution's gather, per forward
    of ``net`` on levels of ``rows`` voxels: (training_graph, one_launch), counted as ``scripts/bench_hrnet.infer_bytes`` does.  With
    e = 4 n c for an (n, c) map — training graph in eval mode: a fused convolution writes z (e) and ``bn_act`` reads every z of its
    sum and the residual and writes y; an octant convolution writes z, ATen's BatchNorm reads and writes it, ``F.relu`` again (5 e); a
    block that reads more than 256 columns forms each of its two sums with ``cat_conv3d`` (two z written, both read, one written: 5
    e), ATen's BatchNorm (2 e) and, for ``conv1``, ``F.relu`` (2 e); a narrower decoder block's ``torch.cat`` reads and writes its
    input once.  One launch: every launch writes y and reads its residual; the second launch of a chain reads and writes the sum."""
    from csn_amd.minkowski_unet import UNetBasicBlock
    two = one = 0
    P = net.PLANES
    e = lambda level, c: 4 * rows[level] * c

    def blocks(seq, level):
        nonlocal two, one
        for blk in seq:
            c = blk.norm2.num_features
            if isinstance(blk, UNetBasicBlock):
                if blk.inplanes > 256:
                    two += (5 + 2 + 2) * e(level, c) + (5 + 2) * e(level, c)    # conv1: cat_conv3d, norm, relu; downsample: cat_conv3d, norm
                    one += 2 * 3 * e(level, c)                                  # two chains: y written, read and written again
                else:
                    two += 3 * e(level, c) + e(level, c)                        # conv1: z w, z r, y w; downsample: z w
                    one += 2 * e(level, c)                                      # two launches: y written
                two += (2 + 2) * e(level, c)                                    # conv2: z w; bn_act: two z (or z and the map) r, y w
                one += 2 * e(level, c)                                          # the residual read, y written
            else:
                two += 3 * e(level, c) + 4 * e(level, c)                        # conv1: z w, z r, y w; conv2: z w, z r, x r, y w
                one += e(level, c) + 2 * e(level, c)
    two += 3 * e(0, net.INIT_DIM)
    one += e(0, net.INIT_DIM)
    c = net.INIT_DIM
    for n in (1, 2, 3, 4):
        two += 5 * e(n, c)
        one += e(n, c)
        blocks(getattr(net, f"block{n}"), n)
        c = P[n - 1]
    skips = (P[2], P[1], P[0], net.INIT_DIM)
    for n in (4, 5, 6, 7):
        level = 7 - n
        two += 5 * e(level, P[n])
        one += e(level, P[n])
        if P[n] + skips[n - 4] <= 256:
            two += 2 * e(level, P[n] + skips[n - 4])                            # torch.cat: read + write
        blocks(getattr(net, f"block{n + 1}"), level)
    return two, one


ROUTES16 = {"fp32_maps": {}, "octant16": {"octant_single_product": True}, "maps16": {"unet_maps16": True}}


def count_bytes_16(forward):
    """One forward with ``sparse_conv_bn_act`` and ``octant_conv_bn_act`` wrapped: the bytes of every launch's maps by their own
    element size.  A down convolution gathers every fine row once, an up convolution one coarse row per fine row."""
    from csn_amd import minkowski_hrnet as MH
    from csn_amd import minkowski_unet as MU
    conv, octant = MH.sparse_conv_bn_act, MU.octant_conv_bn_act
    tot = {"gathered": 0, "written": 0, "residual": 0}

    def add(rows, x, y, residual):
        tot["gathered"] += rows * (-(-x.shape[1] // 32) * 32) * x.element_size()
        tot["written"] += y.numel() * y.element_size()
        tot["residual"] += 0 if residual is None else residual.numel() * residual.element_size()

    def counted(x, weight, kmap, norm, residual=None, relu=True, out=None, **kw):
        y = conv(x, weight, kmap, norm, residual, relu, out, **kw)
        add(int((kmap.fwd >= 0).sum()), x, y, residual)
        return y

    def counted_octant(x, weight, omap, norm, up, residual=None, relu=True, out=None, **kw):
        y = octant(x, weight, omap, norm, up, residual, relu, out, **kw)
        add(omap.n_fine, x, y, residual)
        return y
    MH.sparse_conv_bn_act = MU.sparse_conv_bn_act = counted
    MU.octant_conv_bn_act = counted_octant
    try:
        forward()
    finally:
        MH.sparse_conv_bn_act = MU.sparse_conv_bn_act = conv
        MU.octant_conv_bn_act = octant
    return tot


def faster16(r, new, old="fp32_maps"):
    gap = r[f"{old}_ms"] - r[f"{new}_ms"]
    noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in (new, old))
    r[f"{new}_speedup"] = r[f"{old}_ms"] / r[f"{new}_ms"]
    r[f"{new}_is_faster"] = bool(gap > noise and r[f"{new}_spread_ms"][1] < r[f"{old}_spread_ms"][0])


def infer(a):
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib, build_unet_pyramid, tuning
    from csn_amd import functional as CF
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_unet_pyramid(coords)
    n = coords.shape[0]
    rows = [int(c.shape[0]) for c in pyr.coords]
    res = {"voxels": int(n), "level_rows": rows, "shapes": a.shapes, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "what": "Res16UNet forward, eval, no_grad: eval_epilogue off against on"}
    feats = torch.randn(n, 3, device="cuda")
    for name in ("Res16UNet34C", "Res16UNet14"):
        net = getattr(csn_amd, name)(3, 16).cuda().eval()

        def step_of(mode, on):
            def step():
                with torch.no_grad(), CF.math_mode(CF.mode_id(mode)), tuning.override(eval_epilogue=on):
                    net((pyr, feats))
            return step
        two, one = infer_bytes(net, rows)
        calls = {}
        for v, on in (("training_graph", False), ("one_launch", True)):
            count = [0]
            _lib.set_call_hook(lambda _name, phase: count.__setitem__(0, count[0] + (phase == "begin")))
            try:
                step_of("bf16x3", on)()
            finally:
                _lib.set_call_hook(None)
            calls[v] = count[0]
        res[name] = {"counted_bytes": {"training_graph": two, "one_launch": one}, "library_calls": calls}
        for mode in ("fp32", "bf16x3"):
            r = compare({"training_graph": step_of(mode, False), "one_launch": step_of(mode, True)}, a.warmup, a.iters, a.rounds)
            gap = r["training_graph_ms"] - r["one_launch_ms"]
            noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in ("training_graph", "one_launch"))
            r["speedup"] = r["training_graph_ms"] / r["one_launch_ms"]
            r["one_launch_is_faster"] = bool(gap > noise and r["one_launch_spread_ms"][1] < r["training_graph_spread_ms"][0])
            res[name][f"eval_fwd_{mode}"] = r

        def step16_of(mode, route):
            def step():
                with torch.no_grad(), CF.math_mode(CF.mode_id(mode)), tuning.override(eval_epilogue=True, rows_single_product=True,
                                                                                      **ROUTES16[route]):
                    net((pyr, feats))
            return step
        res[name]["counted_bytes_16"] = {v: count_bytes_16(step16_of("bf16", v)) for v in ROUTES16}
        for mode in ("bf16", "fp16"):
            r = compare({v: step16_of(mode, v) for v in ROUTES16}, a.warmup, a.iters, a.rounds)
            faster16(r, "octant16")
            faster16(r, "maps16")
            res[name][f"eval_fwd_{mode}"] = r
    return res


def train(a):
    """``--train``: the training step (forward + backward) of ``Res16UNet34C`` and ``Res16UNet14`` in math modes bf16x3 and fp32, three
    columns in the same alternating rounds: ``unfused`` (``fused=False``), ``fused`` and ``fused_tail`` (``fused=True`` under
    ``tuning.unet_fused_tail``: the resolution changes and the wide blocks' first convolutions on the fused nodes too)."""
    import csn_amd
    csn_amd.build()
    from csn_amd import build_unet_pyramid, tuning
    from csn_amd import functional as CF
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_unet_pyramid(coords)
    n = coords.shape[0]
    res = {"voxels": int(n), "level_rows": [int(c.shape[0]) for c in pyr.coords], "shapes": a.shapes, "warmup": a.warmup, "iters": a.iters,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "what": "Res16UNet training forward + backward: fused=False, fused, fused with unet_fused_tail"}
    feats, dy = torch.randn(n, 3, device="cuda"), torch.randn(n, 16, device="cuda")
    for name in ("Res16UNet34C", "Res16UNet14"):
        nets = {"fused": getattr(csn_amd, name)(3, 16, fused=True).cuda().train(), "unfused": getattr(csn_amd, name)(3, 16, fused=False).cuda().train()}
        nets["unfused"].load_state_dict(nets["fused"].state_dict())
        res[name] = {"wide_blocks": [getattr(nets["fused"], f"block{i}")[0].inplanes for i in range(5, 9)
                                     if getattr(nets["fused"], f"block{i}")[0].inplanes > 256]}

        def step_of(mode, net, tail):
            def step():
                for p in net.parameters():
                    p.grad = None
                with CF.math_mode(CF.mode_id(mode)), tuning.override(unet_fused_tail=tail):
                    net((pyr, feats)).backward(dy)
            return step
        for mode in ("bf16x3", "fp32"):
            r = compare({"unfused": step_of(mode, nets["unfused"], False), "fused": step_of(mode, nets["fused"], False),
                         "fused_tail": step_of(mode, nets["fused"], True)}, a.warmup, a.iters, a.rounds)
            gap = r["fused_ms"] - r["fused_tail_ms"]
            noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in ("fused", "fused_tail"))
            r["fused_tail_gain_ms"] = gap
            r["fused_tail_speedup"] = r["fused_ms"] / r["fused_tail_ms"]
            r["fused_tail_is_faster"] = bool(gap > noise and r["fused_tail_spread_ms"][1] < r["fused_spread_ms"][0])
            res[name][f"train_fwd_bwd_{mode}"] = r
    return res


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
    ap.add_argument("--infer", action="store_true", help="time the eval variants instead: eval_epilogue off against on in fp32 and bf16x3, and the one-launch graph's "
                                                    "fp32-map, single-product-octant and 16-bit-map routes in bf16 and fp16")
    ap.add_argument("--train", action="store_true", help="time the training step instead: fused=False, fused and fused with unet_fused_tail, "
                                                    "Res16UNet34C and Res16UNet14, bf16x3 and fp32")
    a = ap.parse_args()
    if a.infer or a.train:
        line = json.dumps(infer(a) if a.infer else train(a))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
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

            from csn_amd import tuning

            def step_of(net, tail=False):
                def step():
                    for p in net.parameters():
                        p.grad = None
                    with tuning.override(unet_fused_tail=tail):
                        net((pyr, feats)).backward(dy)
                return step
            steps = {v: step_of(net) for v, net in nets.items()}
            steps["fused_tail"] = step_of(nets["fused"], True)
            res["Res16UNet34C_train_fwd_bwd"] = compare(steps, a.warmup, a.iters, a.rounds)
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
