#!/usr/bin/env python3
"""Top-K shape retrieval with and without the fp16 screen (csn_amd.minkowski_csn.topk_retrieval_ragged / knn_graph_screened
against the all-pairs fp32 measure), on clustered synthetic shapes:
  head    64 ragged shapes of 3000-5000 points, C = 256, K = 3 (the MinkowskiNet head's shape graph)
  midfc   16 x 16 shapes of 10 000 points, C = 256, K = 3 (MID-FC's get_knn_graph)
One process, both flows alternating, HIP events, one warm-up round, then the median and the min-max spread of the rounds.
Prints one JSON line and writes it to profiles/retrieval_screen_bench.json.  The share of pairs re-scored is that of THIS
synthetic input; on real PartNet features it is not measured."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csn_amd import functional as CF          # noqa: E402
from csn_amd import minkowski_csn as M        # noqa: E402

PEAK16, PEAK32 = 2500.0, 157.3                # TFLOP/s: dense fp16 and fp32 matrix peaks of the MI355X


def clustered(rng, lens, C, n_clusters=8, parts=12, noise=0.3):
    """Shapes of ``n_clusters`` families scattered around their family's part directions (device rows + offsets)."""
    g = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    dirs = torch.randn((n_clusters, parts, C), device="cuda", generator=g)
    rows, off = [], [0]
    for s, n in enumerate(lens):
        pick = torch.randint(0, parts, (n,), device="cuda", generator=g)
        rows.append(dirs[s % n_clusters][pick] + noise * torch.randn((n, C), device="cuda", generator=g))
        off.append(off[-1] + n)
    return torch.cat(rows), off


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def run(name, flows, rounds):
    """flows: {label: fn}; every round runs each flow once, in turn; the first round is the warm-up."""
    times = {k: [] for k in flows}
    last = {}
    for r in range(rounds + 1):
        for k, fn in flows.items():
            ms, last[k] = timed(fn)
            if r:
                times[k].append(ms)
    return {k: summary(v) for k, v in times.items()}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_screen_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    C, K = 256, 3
    res = {"rounds": a.rounds, "C": C, "K": K}

    # ---- the head's shape graph: ragged shapes ----
    lens = [int(v) for v in rng.integers(3000, 5001, a.shapes)]
    f, off = clustered(rng, lens, C)
    flops = 2.0 * sum(lens) ** 2 * C
    flows = {"screen_kernel": lambda: M.retrieval_screen_ragged(f, off, f, off),
             "exact_kernel": lambda: M.retrieval_measure_ragged(f, off, f, off),
             "exact_all_pairs": lambda: M.topk_neighbors(M.retrieval_measure_ragged(f, off, f, off).cpu(), K, True),
             "through_screen": lambda: M.topk_retrieval_ragged(f, off, f, off, K, True)}
    t, last = run("head", flows, a.rounds)
    nb, stats = last["through_screen"]
    assert nb == last["exact_all_pairs"], "the screened graph differs from the all-pairs graph"
    head = {"shapes": a.shapes, "points": sum(lens), "times": t, "stats": stats,
            "rescored_share": stats["pairs_rescored"] / stats["pairs_screened"],
            "screen_tflops": flops / t["screen_kernel"]["median_ms"] / 1e9,
            "exact_tflops": flops / t["exact_kernel"]["median_ms"] / 1e9}
    head["kernel_ratio"] = t["exact_kernel"]["median_ms"] / t["screen_kernel"]["median_ms"]
    head["screen_of_fp16_peak"] = head["screen_tflops"] / PEAK16
    head["exact_of_fp32_peak"] = head["exact_tflops"] / PEAK32
    head["speedup_median"] = t["exact_all_pairs"]["median_ms"] / t["through_screen"]["median_ms"]
    head["speedup_worst_case"] = t["exact_all_pairs"]["min_ms"] / t["through_screen"]["max_ms"]
    res["head"] = head
    del f

    # ---- MID-FC: fixed-length shapes ----
    S, N = 16, 10000
    g, _ = clustered(rng, [N] * S, C)
    g = g.reshape(S, N, C)
    flows = {"exact_kernel": lambda: CF.retrieval_measure(g, g),
             "exact_all_pairs": lambda: CF.retrieval_measure(g, g).topk(K + 1, -1)[1],
             "through_screen": lambda: M.knn_graph_screened(g, g, K)}
    t, last = run("midfc", flows, a.rounds)
    idx, stats = last["through_screen"]
    assert torch.equal(idx, last["exact_all_pairs"]), "the screened graph differs from the all-pairs graph"
    mid = {"shapes": S, "points_per_shape": N, "times": t, "stats": stats,
           "rescored_share": stats["pairs_rescored"] / stats["pairs_screened"],
           "exact_tflops": 2.0 * (S * N) ** 2 * C / t["exact_kernel"]["median_ms"] / 1e9,
           "speedup_median": t["exact_all_pairs"]["median_ms"] / t["through_screen"]["median_ms"],
           "speedup_worst_case": t["exact_all_pairs"]["min_ms"] / t["through_screen"]["max_ms"]}
    res["midfc"] = mid
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
