"""Time the METRIC WORK of one MID-FC validation batch — the loss and the Part-IoU counts of a batch of logits — on two paths in one
process:

  fused   ``csn_amd.functional.masked_ce_metrics`` (include/csn_hip.h section 10, csn_masked_ce_metrics_fwd_f32) + the sum of its
          per-shape counts (``training._iou_from_counts``): what ``training.validate_layers`` runs per batch on the device;
  parent  the composition it replaces: ``masked_cross_entropy`` + the torch statements of ``IoU_per_shape``
          (``training._iou_per_shape_torch``: transpose + copy, ``torch.where`` — a ``nonzero``, so a host synchronisation — gather,
          arg-max, two (class_num, points) boolean matrices and their sums).

Logits of configuration 3: ``--shapes`` (32) x ``--classes`` (39) x ``--points`` (10 000) fp32, labels uniform in 0 .. classes - 1.
Device EVENTS around ``--calls`` (20) calls in a row, ``--rounds`` (5) rounds per path, the paths alternating, after ``--warmup`` (5)
calls of each: the figure is the median over the rounds of the time per call, ``spread`` its minimum and maximum.  The parent's host
synchronisation lies inside its window, as it does in a validation loop.  Both paths are first checked to agree exactly.  There is
no threshold: both figures are recorded, and whether their spreads overlap.  Needs the device; prints one JSON line.

    python scripts/bench_midfc_metrics.py --out profiles/midfc_metrics_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# passes over logits-sized data, by name (39 classes x 320 000 points x 4 bytes = 50 MB each)
PASSES = {
    "fused": {"reads": ["metrics kernel"], "writes": []},
    "parent": {"reads": ["masked cross-entropy kernel", "permute + reshape copy", "gather of the labelled rows", "arg-max of the gathered rows"],
               "writes": ["permute + reshape copy", "gathered rows"]},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=32)
    ap.add_argument("--classes", type=int, default=39)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_midfc_metrics.py measures on the MI355X: no device found (nothing is measured on the CPU)")
    if a.calls < 20 or a.rounds < 1:
        raise SystemExit("at least 20 calls per round")
    import csn_amd
    csn_amd.build()
    from csn_amd import training as T
    from csn_amd.functional import masked_ce_metrics, masked_cross_entropy

    rng = np.random.default_rng(0)
    S, C, N = a.shapes, a.classes, a.points
    logits = torch.from_numpy(rng.standard_normal(size=(S, C, N, 1)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, C, size=(S, N)).astype(np.int64)).cuda()

    def fused():
        loss, _, _, _, counts = masked_ce_metrics(logits, labels, 0, want_pred=False)
        return (loss,) + T._iou_from_counts(counts, C)

    def parent():
        loss = masked_cross_entropy(logits, labels, 0)[0]
        return (loss,) + T._iou_per_shape_torch(logits, labels, C)

    paths = {"fused": fused, "parent": parent}
    with torch.no_grad():
        for x, y in zip(fused(), parent()):
            assert torch.equal(x, y), "the two paths disagree"
        for _ in range(a.warmup):
            for f in paths.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, f in paths.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.calls):
                    f()
                t1.record()
                t1.synchronize()
                ms[k].append(t0.elapsed_time(t1) / a.calls)

    res = {"what": "metric work of one MID-FC validation batch: loss + Part-IoU counts", "device": torch.cuda.get_device_name(0),
           "logits": [S, C, N], "labels": f"uniform in 0..{C - 1}", "mask": 0, "timer": "device events", "warmup_calls": a.warmup,
           "calls_per_round": a.calls, "rounds": a.rounds}
    for k in paths:
        res[k] = {"ms_per_call": statistics.median(ms[k]), "spread": [min(ms[k]), max(ms[k])], "rounds_ms": ms[k],
                  "logit_sized_reads": len(PASSES[k]["reads"]), "logit_sized_writes": len(PASSES[k]["writes"]), "passes": PASSES[k],
                  "host_synchronisations_per_call": 0 if k == "fused" else 1}
    res["parent_over_fused"] = res["parent"]["ms_per_call"] / res["fused"]["ms_per_call"]
    res["spreads_overlap"] = not (res["fused"]["spread"][1] < res["parent"]["spread"][0] or res["parent"]["spread"][1] < res["fused"]["spread"][0])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
