"""Time ``build_pyramid(voxel_coords, 3, 5)`` under its two backends in one process: ``"torch"`` (one ``searchsorted`` per kernel
offset in torch ops) and ``"hip"`` (include/csn_hip.h section 17 around ``torch.sort`` / ``torch.unique``).

Field: that of scripts/bench_field.py — ``--shapes`` (8) synthetic ellipsoid shells of ``--points`` (10 000) surface points each, the
voxel size bisected until the field has about ``--voxels`` (32 768) voxels.  The timer is the WALL CLOCK between two
``torch.cuda.synchronize()`` calls around one build: the torch backend is bound by launches and host reads, which device events
around it would not see.  Both backends are warmed up, then timed in ``--rounds`` (5) alternating rounds of ``--iters`` (20) builds:
the figure is the median over the rounds of each round's median, ``spread`` its min and max over the rounds.  ``hip_faster`` is true
when the hip median is below the torch one by more than the larger of the two spreads.  The two pyramids are compared table by
table first.  ``backbone_3s_step_ms`` is quoted from profiles/hrnet_bench.json when that file is there (the network the pyramid
feeds).  Prints one JSON line.

``--only hip|torch`` runs one backend and skips the comparison (a profiler pass wants one).  ``--breakdown FILE --out JSON`` measures
nothing: it reads the kernel statistics CSV of such a pass (``rocprofv3 --kernel-trace --stats``, no counters in that run) and adds the
device time of the native build by kind of launch — the section 17 kernels, the sorts, the unique, the rest — to the JSON file that
an earlier run wrote, per build (``--breakdown-builds``: the builds the profiled run made, its ``builds_per_backend``).

    python scripts/bench_kernel_map.py --out profiles/kernel_map_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -o hip -- python scripts/bench_kernel_map.py --only hip
    python scripts/bench_kernel_map.py --breakdown DIR/.../hip_kernel_stats.csv --breakdown-builds 105 --out profiles/kernel_map_bench.json
"""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KINDS = ("keys", "map", "sort", "unique", "other")


def kind_of(name):
    """The kind of launch a kernel of the native build belongs to, by the names the profiler shows for it on ROCm: the section 17
    kernels by their own names; ``torch.sort`` as rocprim's KEY-VALUE block sort and odd-even block merges (the values are the
    ``OpaqueType<8>`` row numbers) after ``fill_reverse_indices_kernel``; ``torch.unique`` as rocprim's KEY-ONLY sort and merges
    (``empty_type`` values), the ``partition_kernel`` that keeps the first of equal neighbours, its ``init_lookback_scan_state_kernel``
    and the ``transform_kernel`` that copies the count; everything else (unpack, casts, fills, copies, the one-off field build)."""
    if "coord_keys_kernel" in name or "coord_down_kernel" in name:
        return "keys"
    if "kernel_map_kernel" in name:
        return "map"
    if "radix_sort_block_sort_kernel" in name or "device_block_merge_oddeven_kernel" in name:
        return "sort" if "OpaqueType<8>" in name else "unique"
    if "fill_reverse_indices_kernel" in name:
        return "sort"
    if "partition_kernel" in name or "init_lookback_scan_state_kernel" in name or "rocprim" in name and "transform_kernel" in name:
        return "unique"
    return "other"


def wall_round(fn, iters):
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


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
    if "hip_ms" in out and "torch_ms" in out:
        noise = max(out["hip_spread_ms"][1] - out["hip_spread_ms"][0], out["torch_spread_ms"][1] - out["torch_spread_ms"][0])
        out["torch_over_hip"] = out["torch_ms"] / out["hip_ms"]
        out["hip_faster"] = bool(out["hip_ms"] + noise < out["torch_ms"])
    return out


def breakdown(path, builds):
    """Device microseconds per build by kind of launch, from a kernel statistics CSV (columns Name, Calls, TotalDurationNs)."""
    kinds = {k: {"us_per_build": 0.0, "launches_per_build": 0.0} for k in KINDS}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            kind = kind_of(row.get("Name") or row.get("KernelName") or "")
            kinds[kind]["us_per_build"] += float(row["TotalDurationNs"]) / 1e3 / builds
            kinds[kind]["launches_per_build"] += float(row["Calls"]) / builds
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--stem", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="hip or torch: run that backend alone")
    ap.add_argument("--breakdown", default=None, help="kernel statistics CSV of a profiler pass over --only hip")
    ap.add_argument("--breakdown-builds", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.breakdown:
        if not (a.out and os.path.exists(a.out) and a.breakdown_builds > 0):
            raise SystemExit("--breakdown needs --out (the JSON file of an earlier run) and --breakdown-builds")
        with open(a.out) as fh:
            res = json.loads(fh.readline())
        res["hip_device_time_per_build"] = breakdown(a.breakdown, a.breakdown_builds)
        res["hip_device_time_per_build"]["source"] = "rocprofv3 --kernel-trace --stats over --only hip, %d builds" % a.breakdown_builds
        line = json.dumps(res)
        print(line)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_kernel_map.py measures on the device: no device found")
    import csn_amd
    csn_amd.build()
    from bench_field import field_at, shell_points
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
    coords = field_at(shapes, feats, mid, "cuda").voxel_coords
    res = {"voxels": coords.shape[0], "shapes": a.shapes, "levels": a.levels, "stem_kernel": a.stem, "voxel_size": mid,
           "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "timer": "wall clock between two device synchronisations",
           "device": torch.cuda.get_device_name(0)}
    maps = lambda p: p.s1 + [p.stem] + p.down
    if not a.only:
        hip, ref = build_pyramid(coords, a.levels, a.stem, backend="hip"), build_pyramid(coords, a.levels, a.stem, backend="torch")
        same = all(torch.equal(x, y) for x, y in zip(hip.coords, ref.coords))
        for x, y in zip(maps(hip), maps(ref)):
            same = same and torch.equal(x.fwd, y.fwd) and (x.bwd_table is None) == (y.bwd_table is None) and torch.equal(x.bwd, y.bwd)
        res["pyramids_equal"] = bool(same)
        res["level_voxels"] = [c.shape[0] for c in hip.coords]
        res["table_entries"] = sum(m.fwd.numel() + (0 if m.bwd_table is None else m.bwd_table.numel()) for m in set(maps(hip)))
    variants = {"hip": lambda: build_pyramid(coords, a.levels, a.stem, backend="hip"),
                "torch": lambda: build_pyramid(coords, a.levels, a.stem, backend="torch")}
    variants = {v: f for v, f in variants.items() if not a.only or v == a.only}
    res["build_pyramid"] = compare(variants, a.warmup, a.iters, a.rounds)
    res["builds_per_backend"] = (0 if a.only else 1) + a.warmup + a.iters * a.rounds      # the comparison built each pyramid once
    bench = os.path.join(ROOT, "profiles", "hrnet_bench.json")
    if os.path.exists(bench):
        with open(bench) as fh:
            res["backbone_3s_step_ms"] = json.loads(fh.readline()).get("backbone_3S_train_fwd_bwd", {}).get("fused_ms")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
