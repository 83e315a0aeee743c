#!/usr/bin/env python3
"""Time ``build_unet_pyramid(coords, 5)`` — what a ``Res16UNet*`` step that starts from coordinates builds first — in one process
under three configurations, and one ``Res16UNet34C`` training step that includes it.  Development aid, not the headline bench.

  torch     ``backend="torch"``: every kernel map and every octant map from torch ops.
  mixed     the best the parent commit had: the eleven kernel maps through ``build_kernel_map(backend="hip")`` (include/csn_hip.h
            section 17, each call packing and sorting its level's keys again and reading its own status word) around torch octant
            maps.  Restated here, because the tuning switch now selects the native octant maps as well.
  hip       ``backend="hip"``: sections 17 and 22, every level's keys and sort formed once, one host read.

Voxels: the ``--voxels`` (32 768) of scripts/bench_unet.py — 8 synthetic ellipsoid shells (scripts/bench_sparse_conv.py).  The
timer is the WALL CLOCK between two ``torch.cuda.synchronize()`` calls around one build (or one step): the torch backend is bound
by launches and host reads, which device events around it would not see.  Every configuration is warmed up, then timed in
``--rounds`` alternating rounds of ``--iters`` builds: the figure is the median over the rounds of each round's median, ``spread``
its min and max over the rounds.  ``hip_faster_than_mixed`` / ``hip_faster_than_torch`` are true when the hip median lies below the
other by more than the larger of the two spreads.  The three pyramids are compared tensor by tensor first.  The step is
``Res16UNet34C(3, 16)`` in training mode, forward + backward from COORDINATES (the model builds its pyramid), under ``torch`` and
under ``hip`` (``tuning.override(native_kernel_maps=True)``); ``step_without_build_ms`` is the same step on a pyramid built
outside the window.  Prints one JSON line.

    python scripts/bench_unet_pyramid.py --out profiles/unet_pyramid_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_kernel_map import wall_round  # noqa: E402
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def compare(variants, warmup, iters, rounds):
    samples = {v: [] for v in variants}
    for rnd in range(rounds + 1):                                       # round 0 is the warm-up
        for v, fn in variants.items():
            t = wall_round(fn, warmup if rnd == 0 else iters)
            if rnd:
                samples[v].append(t)
    out = {}
    for v, s in samples.items():
        out[f"{v}_ms"] = statistics.median(s)
        out[f"{v}_spread_ms"] = [min(s), max(s)]
    for other in variants:
        if other != "hip" and "hip" in variants:
            noise = max(out["hip_spread_ms"][1] - out["hip_spread_ms"][0], out[f"{other}_spread_ms"][1] - out[f"{other}_spread_ms"][0])
            out[f"{other}_over_hip"] = out[f"{other}_ms"] / out["hip_ms"]
            out[f"hip_faster_than_{other}"] = bool(out["hip_ms"] + noise < out[f"{other}_ms"])
    return out


def mixed_pyramid(coords, stem_kernel):
    """``build_unet_pyramid`` as the parent commit ran it under ``native_kernel_maps``: native kernel maps, torch octant maps."""
    from csn_amd import UNetPyramid, build_kernel_map, build_octant_map
    levels, s1, one, octs = [coords.long()], [], [], []
    for l in range(5):
        ts = 1 << l
        s1.append(build_kernel_map(levels[l], kernel_size=3, stride=1, tensor_stride=ts, backend="hip"))
        one.append(build_kernel_map(levels[l], kernel_size=1, stride=1, tensor_stride=ts, backend="hip"))
        if l + 1 < 5:
            octs.append(build_octant_map(levels[l], tensor_stride=ts, backend="torch"))
            levels.append(octs[-1].out_coords)
    stem = s1[0] if stem_kernel == 3 else build_kernel_map(levels[0], kernel_size=stem_kernel, stride=1, tensor_stride=1, backend="hip")
    return UNetPyramid(levels, s1, one, stem, octs, stem_kernel)


def tensors_of(p):
    out = list(p.coords)
    for m in p.s1 + p.one + [p.stem]:
        out.append(m.fwd)
    for m in p.oct:
        out += [m.in_coords, m.out_coords, m.parent, m.octant, m.children, m.order, m.seg]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--stem", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet_pyramid.py measures on the device: no device found")
    import csn_amd
    csn_amd.build()
    from csn_amd import Res16UNet34C, build_unet_pyramid, tuning
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    n = coords.shape[0]
    res = {"voxels": int(n), "shapes": a.shapes, "stem_kernel": a.stem, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "timer": "wall clock between two device synchronisations", "device": torch.cuda.get_device_name(0)}
    builds = {"torch": lambda: build_unet_pyramid(coords, a.stem, backend="torch"),
              "mixed": lambda: mixed_pyramid(coords, a.stem),
              "hip": lambda: build_unet_pyramid(coords, a.stem, backend="hip")}
    built = {v: tensors_of(f()) for v, f in builds.items()}
    res["pyramids_equal"] = bool(all(len(built[v]) == len(built["torch"]) and all(torch.equal(x, y) for x, y in zip(built[v], built["torch"]))
                                     for v in ("mixed", "hip")))
    res["level_rows"] = [int(c.shape[0]) for c in built["hip"][:5]]
    del built
    res["build_unet_pyramid"] = compare(builds, a.warmup, a.iters, a.rounds)

    if not a.skip_network:
        net = Res16UNet34C(3, 16, conv1_kernel_size=a.stem).cuda().train()
        feats = torch.randn(n, 3, device="cuda")
        dy = torch.randn(n, 16, device="cuda")

        def step_of(where, native):
            def step():
                for p in net.parameters():
                    p.grad = None
                with tuning.override(native_kernel_maps=native):
                    net((where, feats)).backward(dy)
            return step
        r = compare({"torch": step_of(coords, False), "hip": step_of(coords, True)}, a.warmup, a.iters, a.rounds)
        pyr = build_unet_pyramid(coords, a.stem, backend="hip")
        r.update({"step_without_build_" + k[len("hip_"):]: v for k, v in compare({"hip": step_of(pyr, True)}, a.warmup, a.iters, a.rounds).items()})
        res["Res16UNet34C_train_step_from_coordinates"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
