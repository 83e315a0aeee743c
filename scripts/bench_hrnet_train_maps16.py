"""Time and size the HRNet3S training step on fp32 maps against bf16 maps (``tuning.train_maps16``; include/csn_hip.h section 28) in math
mode bf16 with ``rows_single_product``: the backbone's forward + backward on ``--voxels`` (32768) voxels of 8 synthetic ellipsoid
shells from a fixed ``dy``, the pyramid built once outside the timed window.

    fp32_maps   the switch off: sections 14 / 15 per layer, every map fp32 (the parent's route)
    maps16      the switch on: section 28, the ReLU outputs between the layers bf16 rows

HIP events around each step; every variant is warmed up (``--warmup``, 5 steps), then timed in ``--rounds`` (5) alternating rounds of
``--iters`` steps: the figure is the median over the rounds of each round's median, ``spread`` its min and max
(scripts/bench_hrnet.py ``compare``).  ``maps16_is_faster`` is true only when the medians differ by more than both spreads and the
spreads do not overlap; otherwise no gain is shown.

``max_memory_allocated``: the peak of one step each way on top of what was allocated before it (model, pyramid, inputs).
``per_call_ms``: HIP events around every library call of a step (``_lib.set_call_hook``), the median over 5 steps summed per entry point —
which of the four section-28 calls gains or loses against the call it replaces.
``simcsn_3S_K3``: one ``HRNetSimCSN3S`` training step (forward, loss, backward) with K = 3 key batches on separate backbone passes,
``--csn-voxels`` (8192) voxels per batch, timed the same way.  Prints one JSON line.

    python scripts/bench_hrnet_train_maps16.py --out profiles/hrnet_train_maps16_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_hrnet import compare  # noqa: E402
from scripts.bench_hrnet_maps16 import faster  # noqa: E402
from scripts.bench_sparse_conv import shell_shapes  # noqa: E402


def per_call_ms(_lib, step, reps):
    """HIP events around every library call of ``reps`` steps: the median per call, summed per entry point."""
    events, runs, names = [], [], []

    def hook(name, phase):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.append((name, phase, e))
    for _ in range(reps):
        events.clear()
        _lib.set_call_hook(hook)
        try:
            step()
        finally:
            _lib.set_call_hook(None)
        torch.cuda.synchronize()
        begins, ends = [(n, e) for n, p, e in events if p == "begin"], [e for _, p, e in events if p == "end"]
        names = [n for n, _ in begins]
        runs.append([b.elapsed_time(e) for (_, b), e in zip(begins, ends)])
    med = [statistics.median(r[i] for r in runs) for i in range(len(runs[0]))]
    out = {}
    for n, t in zip(names, med):
        out.setdefault(n, [0, 0.0])
        out[n][0] += 1
        out[n][1] += t
    return {k: {"calls": v[0], "ms": round(v[1], 4)} for k, v in sorted(out.items(), key=lambda kv: -kv[1][1])}


def peak_bytes(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=32768)
    ap.add_argument("--csn-voxels", type=int, default=8192)
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import csn_amd
    csn_amd.build()
    from csn_amd import HRNetBackbone, HRNetSimCSN3S, _lib, build_pyramid
    from csn_amd import functional as CF
    from csn_amd import tuning
    torch.manual_seed(0)
    coords = shell_shapes(a.shapes, a.voxels // a.shapes).cuda()
    pyr = build_pyramid(coords, 3)
    n = coords.shape[0]
    res = {"voxels": int(n), "level_rows": [int(c.shape[0]) for c in pyr.coords], "shapes": a.shapes, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "what": "HRNetBackbone 3S forward + backward, training, math mode bf16 + rows_single_product; maps16 adds train_maps16"}
    feats = torch.randn(n, 3, device="cuda")
    net = HRNetBackbone(3, 3, 2).cuda().train()
    dy = torch.randn(n, net.out_channels, device="cuda")

    def step_of(on):
        def step():
            for p in net.parameters():
                p.grad = None
            with CF.math_mode("bf16"), tuning.override(rows_single_product=True, train_maps16=on):
                net(feats, pyr).backward(dy)
        return step
    steps = {"fp32_maps": step_of(False), "maps16": step_of(True)}
    r = faster(compare(steps, a.warmup, a.iters, a.rounds), "maps16", "fp32_maps")
    r["max_memory_allocated"] = {v: peak_bytes(s) for v, s in steps.items()}
    r["per_call_ms"] = {v: per_call_ms(_lib, s, 5) for v, s in steps.items()}
    res["backbone_3S_train_fwd_bwd_bf16"] = r

    def emit():
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line
    emit()                                                                  # (kept if the second measurement cannot run)

    # one HRNetSimCSN3S step with K = 3 key batches, separate passes
    base = shell_shapes(a.shapes, a.csn_voxels // a.shapes)
    batches = []
    for g in range(4):
        c = (base + torch.tensor([0, 3 * g, -2 * g, g])).cuda()
        batches.append((build_pyramid(c, 3), torch.randn(c.shape[0], 3, device="cuda")))
    model = HRNetSimCSN3S(3, 16, d_model=256, n_head=4, k_neighbors=3, dropout=0.0).cuda().train()

    def csn_step_of(on):
        def step():
            for p in model.parameters():
                p.grad = None
            with CF.math_mode("bf16"), tuning.override(rows_single_product=True, train_maps16=on):
                model(batches[0], batches[1:]).square().mean().backward()
        return step
    csn = {"fp32_maps": csn_step_of(False), "maps16": csn_step_of(True)}
    r = faster(compare(csn, a.warmup, max(a.iters // 2, 3), a.rounds), "maps16", "fp32_maps")
    r["max_memory_allocated"] = {v: peak_bytes(s) for v, s in csn.items()}
    r["voxels_per_batch"] = int(batches[0][1].shape[0])
    res["simcsn_3S_K3_train_step_bf16"] = r
    print(emit())


if __name__ == "__main__":
    main()
