"""Time the DATA SIDE of one MinkowskiNet training step — from drawn augmentation numbers to the four ``PointField``s of a query batch
and its K neighbour batches — on two paths in one process:

  device  ``PointCollection.batch`` / ``neighbor_batches`` + ``PointBatch.field()`` (include/csn_hip.h section 18): the category is
          resident, a batch is two uploads and two launches, a field one sort, one scan, one host read and one launch;
  host    what a user of the package has without it: the category in host memory, per item the numpy chain of
          ``tests/points_ref.reference_item`` (rotation, shift or jitter, scale — the reference's order), ``batch_points``, the copy to
          the device, ``PointField(coords, feats)``.

Step: B = ``--shapes`` (32) query shapes and K = ``--K`` (3) neighbours each, (K + 1) B = 128 items of ``--points`` (10 000) points out
of a category of ``--category`` (256) synthetic shapes (anisotropic Gaussian clouds, normalised to the unit sphere); the numbers are
drawn with ``AugmentSpec.distort_partnet()`` (rotation + jitter + scale, the reference's training setting) inside the timed window
on both paths; voxel size 0.05.  WALL CLOCK between two device synchronisations (the host path is bound by numpy and host reads,
which device events would not see), ``--warmup`` (3) steps, then ``--reps`` (20) alternating steps per path: the figure is the median,
``spread`` its minimum and maximum.  Every step uses its own seeded indices and numbers, the same on both paths.  There is no
threshold: both numbers and their ratio are recorded.  Needs the device; prints one JSON line.

    python scripts/bench_points.py --out profiles/points_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def category(n_shapes, n_points, seed=0):
    from tests import points_ref as R
    shapes = R.random_shapes(n_shapes, n_points, seed=seed)
    return np.stack([R.normalize64(s).astype(np.float32) for s in shapes])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=32)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--category", type=int, default=256)
    ap.add_argument("--voxel-size", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_points.py measures on the MI355X: no device found (nothing is measured on the CPU)")
    import csn_amd
    csn_amd.build()
    from csn_amd import AugmentSpec, PointCollection, PointField, batch_points
    from tests import points_ref as R

    B, K, vs = a.shapes, a.K, a.voxel_size
    host_points = category(a.category, a.points)
    host_labels = np.random.default_rng(1).integers(0, 11, size=(a.category, a.points)).astype(np.int32)
    col = PointCollection(host_points, host_labels)
    spec = AugmentSpec.distort_partnet()
    sigma, clip = spec.shift

    def plan(step):
        rng = np.random.default_rng(1000 + step)
        q = rng.integers(0, a.category, size=B)
        neighbors = [(int(s), rng.integers(0, a.category, size=K).tolist()) for s in q]
        return rng, q, neighbors

    def device_step(step):
        rng, q, neighbors = plan(step)
        p = spec.draw((K + 1) * B, rng)
        fields = [col.batch(q, p.slice(0, B), vs, spec.shift).field()]
        fields += [b.field() for b in col.neighbor_batches(neighbors, K, p.slice(B, (K + 1) * B), vs, spec.shift)]
        return fields

    def host_batch(idx, p):
        items = []
        for i, s in enumerate(idx):
            aug, _ = R.reference_item(host_points[s], p.angle[i], p.shift_z[i], p.jitter[i], p.scale[i], sigma, clip, vs,
                                      shift_on=spec.shift_on, jitter_on=spec.jitter_on)
            items.append((torch.from_numpy(aug), torch.from_numpy(aug.astype(np.float32)), torch.from_numpy(host_labels[s])))
        coords, feats, _ = batch_points(items, vs)
        return PointField(coords.cuda(), feats.cuda())

    def host_step(step):
        rng, q, neighbors = plan(step)
        p = spec.draw((K + 1) * B, rng)
        fields = [host_batch(q, p.slice(0, B))]
        fields += [host_batch([n[1][i] for n in neighbors], p.slice((i + 1) * B, (i + 2) * B)) for i in range(K)]
        return fields

    def wall(fn, step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(step)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # the two paths build the same fields (statement (b) against the reference's order: equal on every point seen so far)
    fd, fh = device_step(0), host_step(0)
    same = all(torch.equal(x.coords, y.coords) and torch.equal(x.feats, y.feats) and torch.equal(x.voxel_coords, y.voxel_coords)
               and torch.equal(x.home, y.home) for x, y in zip(fd, fh))
    samples = {"device": [], "host": []}
    for step in range(a.warmup + a.reps):
        for name, fn in (("device", device_step), ("host", host_step)):
            ms, _ = wall(fn, step + 1)
            if step >= a.warmup:
                samples[name].append(ms)
    res = {"measured": True, "device": torch.cuda.get_device_name(0), "shapes": B, "K": K, "items": (K + 1) * B, "points": a.points,
           "category_shapes": a.category, "voxel_size": vs, "augmentation": "distort_partnet (rotation + jitter + scale)",
           "voxels_per_field": [f.n_voxels for f in fd], "warmup": a.warmup, "reps": a.reps, "clock": "wall, between device synchronisations",
           "fields_equal_on_both_paths": bool(same)}
    for name, s in samples.items():
        res[f"{name}_ms"] = statistics.median(s)
        res[f"{name}_spread_ms"] = [min(s), max(s)]
    res["host_over_device"] = res["host_ms"] / res["device_ms"]
    # where the device path's time goes: the batches alone, then the fields alone on kept batches
    rng, q, neighbors = plan(0)
    p = spec.draw((K + 1) * B, rng)
    make = lambda _: [col.batch(q, p.slice(0, B), vs, spec.shift)] + col.neighbor_batches(neighbors, K, p.slice(B, (K + 1) * B), vs, spec.shift)
    kept = make(0)
    res["device_batches_only_ms"] = statistics.median(wall(make, 0)[0] for _ in range(a.reps))
    res["device_fields_only_ms"] = statistics.median(wall(lambda _: [b.field() for b in kept], 0)[0] for _ in range(a.reps))
    res["draw_only_ms"] = statistics.median(wall(lambda _: spec.draw((K + 1) * B, np.random.default_rng(0)), 0)[0] for _ in range(a.reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh_:
            fh_.write(line + "\n")


if __name__ == "__main__":
    main()
