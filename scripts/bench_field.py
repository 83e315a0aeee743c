"""Time ``PointField.interpolate`` forward + backward (include/csn_hip.h section 16) beside the eager composition of the same map on
the same device in the same process: eight ``index_select`` x weight products, summed, with autograd's ``index_add_`` backward (its
corner rows and weights are formed ONCE outside the timed window, which favours it: the kernels form theirs on every call).

Field: ``--shapes`` (8) synthetic ellipsoid shells of ``--points`` (10 000, PartNet's count) surface points each; the voxel size is
bisected until the field has about ``--voxels`` (32 768) voxels, the size profiles/hrnet_bench.json uses.  C = ``--channels`` (50).
HIP events around each forward + backward; both variants are warmed up, then timed in ``--rounds`` alternating rounds of ``--iters``
steps: the figure is the median over the rounds of each round's median, ``spread`` its min and max over the rounds.
``hip_not_slower`` is true when the HIP median is at most the eager one plus the larger of the two spreads.  For context only: the
``PointField`` build, ``build_pyramid`` on the same voxels (3 levels), the median and maximum points per voxel.  ``--only hip|eager``
runs one variant (a profiler pass wants one).  Prints one JSON line.

    python scripts/bench_field.py --out profiles/field_bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shell_points(n_shapes, per_shape, seed=0):
    """Per shape (per_shape, 3) float64 points on the surface of an ellipsoid with semi-axes near 1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(n_shapes):
        ax = torch.tensor([1.0, 0.8 + 0.05 * s, 1.2 - 0.04 * s], dtype=torch.float64)
        d = torch.randn(per_shape, 3, generator=g, dtype=torch.float64)
        out.append(d / d.norm(dim=1, keepdim=True) * ax)
    return out


def field_at(shapes, feats, voxel_size, device="cpu"):
    from csn_amd import PointField, batch_points
    coords, f = batch_points([(xyz, ft) for xyz, ft in zip(shapes, feats)], voxel_size)
    return PointField(coords.to(device), f.to(device))


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
    samples = {v: [] for v in variants}
    for rnd in range(rounds + 1):                                       # round 0 is the warm-up
        for v, step in variants.items():
            t = timed(step, warmup if rnd == 0 else iters)
            if rnd:
                samples[v].append(t)
    out = {}
    for v, s in samples.items():
        out[f"{v}_ms"] = statistics.median(s)
        out[f"{v}_spread_ms"] = [min(s), max(s)]
    if "hip_ms" in out and "eager_ms" in out:
        noise = max(out["hip_spread_ms"][1] - out["hip_spread_ms"][0], out["eager_spread_ms"][1] - out["eager_spread_ms"][0])
        out["eager_over_hip"] = out["eager_ms"] / out["hip_ms"]
        out["hip_not_slower"] = bool(out["hip_ms"] <= out["eager_ms"] + noise)
    return out


def wall_ms(fn, repeats=3):
    best = math.inf
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="hip or eager: run that variant alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import build_pyramid
    torch.manual_seed(0)
    shapes = shell_points(a.shapes, a.points)
    feats = [torch.randn(a.points, 3) for _ in range(a.shapes)]
    lo, hi = 1e-3, 1.0                                                  # voxels fall as the voxel size grows
    for _ in range(30):
        mid = math.sqrt(lo * hi)
        n = field_at(shapes, feats, mid).n_voxels
        if abs(n - a.voxels) <= a.voxels // 200:
            break
        lo, hi = (mid, hi) if n > a.voxels else (lo, mid)
    voxel_size = mid
    field = field_at(shapes, feats, voxel_size, "cuda")
    counts = (field.vox_ptr[1:] - field.vox_ptr[:-1]).cpu()
    res = {"points": field.n_points, "voxels": field.n_voxels, "shapes": a.shapes, "channels": a.channels, "voxel_size": voxel_size,
           "points_per_voxel_median": float(counts.float().median()), "points_per_voxel_max": int(counts.max()),
           "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    # context: the plumbing around the kernels (wall clock with a synchronisation, best of 3)
    res["point_field_build_ms"] = wall_ms(lambda: field_at(shapes, feats, voxel_size, "cuda").voxel_feats)
    res["build_pyramid_3_levels_ms"] = wall_ms(lambda: build_pyramid(field.voxel_coords, 3))

    C = a.channels
    table = field.corner_table()
    z = torch.randn(field.n_voxels, C, device="cuda", requires_grad=True)
    dy = torch.randn(field.n_points, C, device="cuda")
    # the eager composition's constants
    t = field.coords[:, 1:] - field.coords[:, 1:].floor()
    home = field.home.long()
    idx, wts = [], []
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, c >> 2
        rows = table[13 + cx + 3 * cy + 9 * cz].long()[home]
        w = ((t[:, 0] if cx else 1 - t[:, 0]) * (t[:, 1] if cy else 1 - t[:, 1])) * (t[:, 2] if cz else 1 - t[:, 2])
        idx.append(rows.clamp(min=0))
        wts.append(torch.where(rows >= 0, w, torch.zeros_like(w))[:, None].contiguous())

    def eager_forward(zz):
        y = zz.index_select(0, idx[0]) * wts[0]
        for c in range(1, 8):
            y = y + zz.index_select(0, idx[c]) * wts[c]
        return y

    def hip_step():
        z.grad = None
        field.interpolate(z).backward(dy)

    def eager_step():
        z.grad = None
        eager_forward(z).backward(dy)

    with torch.no_grad():
        res["max_abs_difference_forward"] = float((field.interpolate(z) - eager_forward(z)).abs().max())
    hip_step()
    g_hip = z.grad.clone()
    eager_step()
    res["max_abs_difference_backward"] = float((g_hip - z.grad).abs().max())
    variants = {"hip": hip_step, "eager": eager_step}
    variants = {v: s for v, s in variants.items() if not a.only or v == a.only}
    res["interpolate_fwd_bwd"] = compare(variants, a.warmup, a.iters, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
