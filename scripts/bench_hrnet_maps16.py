"""Time the HRNet3S inference graph on fp32 maps against 16-bit maps (``tuning.infer_maps16``; include/csn_hip.h section 24) in math
modes bf16 and fp16: the backbone forward in eval mode under ``torch.no_grad()`` on ``--voxels`` (32768) voxels of 8 synthetic
ellipsoid shells, the pyramid built once outside the timed window.

    fp32_maps   ``eval_epilogue + rows_single_product``: section 19 per convolution, every map between two launches fp32
    maps16      the same + ``infer_maps16``: section 24 per convolution, the maps between the launches bf16 / fp16 rows

HIP events around each forward; every variant is warmed up, then timed in ``--rounds`` (5) alternating rounds of ``--iters`` forwards:
the figure is the median over the rounds of each round's median, ``spread`` its min and max (scripts/bench_hrnet.py ``compare``).
``maps16_is_faster`` is true only when the medians differ by more than both spreads and the spreads do not overlap.

``counted_bytes``: what the two graphs differ in, counted on the launches themselves (one forward of each variant with
``sparse_conv_bn_act`` wrapped): ``written`` = the output maps, ``residual`` = the residual / running-sum reads, ``gathered`` = (valid
table entries) x c_in x element size — the bytes the gathers use; ``per_conv`` lists them for every convolution.
``per_shape_ms``: HIP events around every library call of one forward (``_lib.set_call_hook``), summed per convolution shape — the
widest layers first.  ``single_launch_64x64_k3``: one 64 -> 64, k = 3 launch on the level-0 map in fp16, fp32 maps (section 19)
against 16-bit maps (section 24, x and y fp16).  Prints one JSON line.

    python scripts/bench_hrnet_maps16.py --out profiles/hrnet_maps16_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_hrnet import compare  # noqa: E402
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def faster(r, new, old):
    gap = r[f"{old}_ms"] - r[f"{new}_ms"]
    noise = max(r[f"{v}_spread_ms"][1] - r[f"{v}_spread_ms"][0] for v in (new, old))
    r["speedup"] = r[f"{old}_ms"] / r[f"{new}_ms"]
    r[f"{new}_is_faster"] = bool(gap > noise and r[f"{new}_spread_ms"][1] < r[f"{old}_spread_ms"][0])
    return r


def count_bytes(MH, forward):
    """One forward with ``sparse_conv_bn_act`` wrapped: the bytes of every launch's maps by their own element size."""
    orig, convs = MH.sparse_conv_bn_act, []

    def counted(x, weight, kmap, norm, residual=None, relu=True, out=None, **kw):
        y = orig(x, weight, kmap, norm, residual, relu, out, **kw)
        valid = int((kmap.fwd >= 0).sum())
        c_in = -(-x.shape[1] // 32) * 32
        convs.append({"kv": int(kmap.KV), "c_in": int(c_in), "c_out": int(y.shape[1]), "n_out": int(y.shape[0]),
                      "gathered": valid * c_in * x.element_size(), "written": y.numel() * y.element_size(),
                      "residual": 0 if residual is None else residual.numel() * residual.element_size()})
        return y
    MH.sparse_conv_bn_act = counted
    try:
        forward()
    finally:
        MH.sparse_conv_bn_act = orig
    tot = {k: sum(c[k] for c in convs) for k in ("gathered", "written", "residual")}
    tot["per_conv"] = [[c["kv"], c["c_in"], c["c_out"], c["n_out"], c["gathered"], c["written"], c["residual"]] for c in convs]
    return tot


def per_shape_ms(_lib, MH, forward, reps):
    """HIP events around every launch of ``reps`` forwards, the median per launch summed per (kv, c_in, c_out, n_out)."""
    orig, shapes, events = MH.sparse_conv_bn_act, [], []

    def named(x, weight, kmap, norm, residual=None, relu=True, out=None, **kw):
        shapes.append((int(kmap.KV), -(-x.shape[1] // 32) * 32, int(weight.shape[2]), int(kmap.n_out)))
        return orig(x, weight, kmap, norm, residual, relu, out, **kw)

    def hook(name, phase):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.append((phase, e))
    runs = []
    MH.sparse_conv_bn_act = named
    try:
        for _ in range(reps):
            shapes.clear()
            events.clear()
            _lib.set_call_hook(hook)
            forward()
            _lib.set_call_hook(None)
            torch.cuda.synchronize()
            begins, ends = [e for p, e in events if p == "begin"], [e for p, e in events if p == "end"]
            runs.append([b.elapsed_time(e) for b, e in zip(begins, ends)])
    finally:
        _lib.set_call_hook(None)
        MH.sparse_conv_bn_act = orig
    med = [statistics.median(r[i] for r in runs) for i in range(len(runs[0]))]
    out = {}
    for s, t in zip(shapes, med):
        key = "kv{} {}->{} n{}".format(*s)
        out.setdefault(key, [0, 0.0])
        out[key][0] += 1
        out[key][1] += t
    return {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in sorted(out.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import HRNetBackbone, _lib, build_pyramid
    from csn_amd import functional as CF
    from csn_amd import minkowski_hrnet as MH
    from csn_amd import tuning
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_pyramid(coords, 3)
    n = coords.shape[0]
    res = {"voxels": int(n), "level_rows": [int(c.shape[0]) for c in pyr.coords], "shapes": a.shapes, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "what": "HRNetBackbone 3S forward, eval, no_grad, eval_epilogue + rows_single_product; maps16 adds infer_maps16"}
    feats = torch.randn(n, 3, device="cuda")
    net = HRNetBackbone(3, 3, 2).cuda().eval()

    def step_of(mode, on):
        def step():
            with torch.no_grad(), CF.math_mode(mode), tuning.override(eval_epilogue=True, rows_single_product=True, infer_maps16=on):
                return net(feats, pyr)
        return step
    for mode in ("bf16", "fp16"):
        steps = {"fp32_maps": step_of(mode, False), "maps16": step_of(mode, True)}
        r = faster(compare(steps, a.warmup, a.iters, a.rounds), "maps16", "fp32_maps")
        r["max_abs_difference"] = float((steps["maps16"]() - steps["fp32_maps"]()).abs().max())
        r["per_shape_ms"] = {v: per_shape_ms(_lib, MH, steps[v], 5) for v in steps}
        res[f"backbone_3S_eval_fwd_{mode}"] = r
    res["counted_bytes"] = {v: count_bytes(MH, step_of("bf16", on)) for v, on in (("fp32_maps", False), ("maps16", True))}

    # one 64 -> 64, k = 3 launch on the level-0 map, fp16: fp32 maps (section 19) against fp16 maps (section 24)
    kmap = pyr.s1[0]
    w = torch.randn(27, 64, 64, device="cuda") / (27 * 64) ** 0.5
    norm = torch.nn.BatchNorm1d(64).cuda().eval()
    x32 = torch.randn(n, 64, device="cuda")
    x16 = x32.half()
    y32, y16 = torch.empty(n, 64, device="cuda"), torch.empty(n, 64, device="cuda", dtype=torch.float16)

    vec = [norm.weight.detach(), norm.bias.detach(), norm.running_mean, norm.running_var]
    lib, st, p = _lib.lib(), torch.cuda.current_stream().cuda_stream, lambda t: t.data_ptr()

    def launch(x, y):
        is16 = int(x.dtype == torch.float16)

        def step():                                                         # the C call alone between the events
            if is16:
                e = lib.csn_sparse_conv_bn_act_fwd_m16(p(x), 1, 64, n, p(kmap.fwd), n, 27, 64, 64, p(w), *(p(v) for v in vec), 1e-5, None, 0,
                                                       0, 1, p(y), 1, 64, st)
            else:
                e = lib.csn_sparse_conv_bn_act_fwd_f32(p(x), 64, n, p(kmap.fwd), n, 27, 64, 64, p(w), *(p(v) for v in vec), 1e-5, None, 0, 1,
                                                       p(y), 64, st)
            _lib.check(e, "single launch")
        return step
    with CF.math_mode("fp16"), CF.rows16(True):
        r = faster(compare({"fp32_maps": launch(x32, y32), "maps16": launch(x16, y16)}, a.warmup, 4 * a.iters, a.rounds), "maps16",
                   "fp32_maps")
    r["rows"] = int(n)
    r["equal_bits"] = bool(torch.equal(y16, y32.half()))
    r["note"] = "HIP events around the C call; x and y fp32 (section 19) against x and y fp16 (section 24), the same values in x"
    res["single_launch_64x64_k3_fp16"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
