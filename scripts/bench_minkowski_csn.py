#!/usr/bin/env python3
"""Throughput of the MinkowskiNet cross-shape head on ragged shape batches (csn_amd/minkowski_csn.py, hrnet.py:359-423) and of
the ragged retrieval measure (hrnet.py:472-490).  Development aid, not the headline bench.

  head       B query shapes of 3000..5000 points (seeded), K neighbour batches, d_model 256, n_head 4, train mode, forward +
             backward with gradients to queries, keys and every parameter: SimCSNHead (one varlen launch chain) against the
             reference's structure — a Python loop of per-shape / per-pair MultiHeadAttention calls plus eager head math.
  retrieval  16 x 16 shapes of 4096 points against csn_retrieval_measure_f32 on the same data, and a ragged 16 x 16 case of
             1000..5000 points in TFLOP/s counting only real point pairs (2 C n m per pair).
  --flows    kept,free: SimCSNHead alone with the kept-scores backward against the score-free one (csn_amd.tuning.cross_score_free),
             alternating in one process: ms per step and the step's peak memory for each.  --points LO,HI sets the shape sizes;
             "auto" leaves the choice to the automatic rule (the capability run at 11000..12000 points).
  --loss     torch,fused: the head's train step (39 classes, ~10 % of the rows labelled 255) with F.cross_entropy(ignore_index=255)
             against csn_amd.seg_loss, alternating step by step in one process: median and interquartile range of --steps
             steps each (>= 20 asked for); then an evaluate loop of 64 single-shape batches (csn_amd.evaluate: no host sync per
             batch) against the reference-style loop on the same logits (cross-entropy, .item(), .cpu().numpy(), calculate_iou
             restated per label on the host)."""
import argparse, os, sys, time
import numpy as np, torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csn_amd import _lib, tuning
from csn_amd import functional as CF
from csn_amd.minkowski_csn import SimCSNHead, retrieval_measure_ragged
from csn_amd.minkowski_training import evaluate, seg_loss


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def loop_step(head, qs, keys):
    """hrnet.py:359-423 as the reference runs it: get_SSA per shape, 2K+1 MHA calls per query shape, eager head math."""
    mha = head.MHA
    ssa = [mha(q[None], q[None], q[None])[0][0] for q in qs]
    K = len(keys)
    key_ssa = [[mha(k[None], k[None], k[None])[0][0] for k in ks] for ks in keys]
    csa = []
    for b, q in enumerate(qs):
        u = F.normalize(head.linear_q(ssa[b].mean(0)), dim=-1)
        sims = [head.sim(u[None], F.normalize(head.linear_k(t.mean(0)), dim=-1)[None]).squeeze()
                for t in [ssa[b]] + [key_ssa[i][b] for i in range(K)]]
        comp = F.softmax(torch.stack(sims), dim=0)
        c = comp[0] * ssa[b]
        for i in range(K):
            c = c + comp[i + 1] * mha(q[None], keys[i][b][None], keys[i][b][None])[0][0]
        csa.append(c)
    return head.output(torch.cat([torch.cat(qs), torch.cat(csa)], 1))


def bench_head(a, mode, K):
    _lib.check(_lib.lib().csn_set_math_mode(mode))
    rng = np.random.default_rng(0)
    H, C = 4, 256
    torch.manual_seed(0)
    head = SimCSNHead(C, H, 39 if a.loss else 20, K).cuda().train()
    lo, hi = (int(x) for x in a.points.split(","))
    lens = lambda: rng.integers(lo, hi + 1, a.shapes).tolist()
    qs = [torch.randn((n, C), device="cuda", requires_grad=True) for n in lens()]
    keys = [[torch.randn((n, C), device="cuda", requires_grad=True) for n in lens()] for _ in range(K)]
    q = torch.cat([t.detach() for t in qs]).requires_grad_(True)
    qo = np.concatenate([[0], np.cumsum([t.shape[0] for t in qs])]).tolist()
    kb = []
    for ks in keys:
        kb.append((torch.cat([t.detach() for t in ks]).requires_grad_(True),
                   np.concatenate([[0], np.cumsum([t.shape[0] for t in ks])]).tolist()))

    def fused():
        head.zero_grad(set_to_none=True)
        head(q, qo, kb).square().mean().backward()

    def loop():
        head.zero_grad(set_to_none=True)
        loop_step(head, qs, keys).square().mean().backward()

    if a.flows:
        return bench_flows(a, mode, K, fused, (lo, hi))
    if a.loss:
        return bench_loss(a, mode, K, head, q, qo, kb, rng)
    ms = timed(fused, a.warmup, a.steps)
    ms_loop = timed(loop, a.warmup, a.steps) if not a.no_loop else float("nan")
    print(f"head mode {'bf16x3' if mode else 'fp32'}: B={a.shapes} shapes of 3000..5000 points, K={K}, d_model={C}, n_head={H}, "
          f"train fwd+bwd: SimCSNHead {ms:8.2f} ms/step, per-pair loop {ms_loop:8.2f} ms/step ({ms_loop / ms:4.2f}x)", flush=True)


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v), [25, 50, 75])
    return f"median {med:8.3f} ms, IQR {q3 - q1:6.3f} ms ({q1:.3f} .. {q3:.3f})"


def bench_loss(a, mode, K, head, q, qo, kb, rng):
    N, n_cls = q.shape[0], 39
    t = rng.integers(0, n_cls, N)
    t[rng.random(N) < 0.1] = 255
    target = torch.from_numpy(t).cuda()
    losses = {"torch": lambda z: F.cross_entropy(z, target, ignore_index=255), "fused": lambda z: seg_loss(z, target, qo, 255)[0]}
    kinds = a.loss.split(",")
    ms = {k: [] for k in kinds}

    def step(kind):
        head.zero_grad(set_to_none=True)
        losses[kind](head(q, qo, kb)).backward()

    for k in kinds:
        for _ in range(a.warmup):
            step(k)
    for _ in range(a.steps):
        for k in kinds:                                      # alternating: drift of the clocks falls on both alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(k)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    for k in kinds:
        print(f"head mode {'bf16x3' if mode else 'fp32'}: B={a.shapes} shapes, {N} rows, K={K}, {n_cls} classes, train step with the "
              f"{k:5s} loss: {quartiles(ms[k])} over {a.steps} steps", flush=True)
    # the loss pair alone on the head's logits (forward + backward to the logits)
    with torch.no_grad():
        z0 = head(q, qo, kb)
    for k in kinds:
        z = z0.clone().requires_grad_(True)
        def pair():
            z.grad = None
            losses[k](z).backward()
        print(f"  {k:5s} loss alone, forward + backward on ({N}, {n_cls}) logits: {timed(pair, a.warmup, max(a.steps, 20)):8.3f} ms", flush=True)


def host_iou(ground, prediction, num_labels):
    """calculate_iou (MinkowskiNet/lib/utils.py:78-110) restated: one host pass over the rows per label."""
    prediction = np.copy(prediction)
    prediction[ground == 0] = 0
    inter, union = {}, {}
    for i in range(1, num_labels):
        u = np.sum((ground == i) | (prediction == i))
        if u > 0:
            inter[i], union[i] = float(np.sum((ground == i) & (prediction == i))), float(u)
    return inter, union


def bench_evaluate(a):
    """64 single-shape test batches of 3000..5000 rows, 39 classes: csn_amd.evaluate against the loop of trainer_csn.py:429-475 on
    the same logits (the model's forward is left out of both)."""
    rng = np.random.default_rng(3)
    n_cls = 39
    batches = []
    for n in rng.integers(3000, 5001, 64).tolist():
        t = rng.integers(0, n_cls, n)
        t[rng.random(n) < 0.1] = 255
        batches.append(((torch.randn((n, n_cls), device="cuda"), [0, n]), torch.from_numpy(t).cuda()))

    def fused():
        return evaluate(lambda b: b, batches, n_cls)

    def reference_style():
        loss_sum = score_sum = rows = 0.0
        inter, union, shape_ious = np.zeros(n_cls), np.zeros(n_cls), []
        for (z, _), target in batches:
            pred = torch.max(z[:, 1:], 1)[1] + 1
            n = target.shape[0]
            loss_sum += float(F.cross_entropy(z, target, ignore_index=255)) * n
            ok = (pred.eq(target) | target.eq(0))[target != 255]
            score_sum += ok.float().sum(0).mul(100.0 / ok.size(0)).item() * n
            rows += n
            i_s, u_s = host_iou(target.cpu().numpy(), pred.cpu().numpy(), n_cls)
            for k in i_s:
                inter[k] += i_s[k]
                union[k] += u_s[k]
            if i_s:
                shape_ious.append(sum(i_s[k] / u_s[k] for k in i_s) / len(i_s))
        part = sum(inter[k] / union[k] if union[k] > 0 else 0.0 for k in range(1, n_cls)) / (n_cls - 1)
        return loss_sum / rows, score_sum / rows, part * 100, float(np.mean(shape_ious)) * 100

    got, want = fused(), reference_style()
    ms = {"evaluate": [], "reference-style": []}
    for _ in range(max(a.steps, 20) // 4 + 1):
        for name, fn in (("evaluate", fused), ("reference-style", reference_style)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    for name in ms:
        print(f"evaluate loop, 64 single-shape batches of 3000..5000 rows, {n_cls} classes, {name:15s}: {quartiles(ms[name])} over "
              f"{len(ms[name])} loops", flush=True)
    print(f"  results (loss, precision, Part IoU, Shape IoU): evaluate {tuple(round(v, 6) for v in got)}, reference-style "
          f"{tuple(round(v, 6) for v in want)}", flush=True)


FLOWS = {"kept": False, "free": True, "auto": None}


def bench_flows(a, mode, K, fused, points):
    flows = a.flows.split(",")
    ms, peak, took = {f: [] for f in flows}, {}, {}
    for _ in range(a.rounds):
        for f in flows:
            names = set()
            with tuning.override(cross_score_free=FLOWS[f]):
                for _ in range(a.warmup):
                    fused()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                _lib.set_call_hook(lambda name, phase: names.add(name))
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fused()
                torch.cuda.synchronize()
                ms[f].append((time.perf_counter() - t0) / a.steps * 1e3)
                _lib.set_call_hook(None)
                peak[f] = max(peak.get(f, 0), torch.cuda.max_memory_allocated() - base)
                took[f] = "score-free" if "csn_varlen_attn_bwd_flash_f32" in names else "kept scores"
    for f in flows:
        print(f"head mode {mode}: B={a.shapes} shapes of {points[0]}..{points[1]} points, K={K}, train fwd+bwd, flow {f:5s} (ran {took[f]}): "
              f"{min(ms[f]):9.2f} ms/step (min of {a.rounds} alternations: {' '.join(f'{x:.1f}' for x in ms[f])}), "
              f"step peak memory {peak[f] / 2 ** 30:7.2f} GiB", flush=True)


def bench_retrieval(a):
    C = 256
    g = torch.Generator(device="cuda").manual_seed(1)
    S, N = 16, 4096
    f1 = torch.randn((S, N, C), device="cuda", generator=g)
    f2 = torch.randn((S, N, C), device="cuda", generator=g)
    off = [i * N for i in range(S + 1)]
    ms_fixed = timed(lambda: CF.retrieval_measure(f1, f2), a.warmup, a.steps)
    ms_rag = timed(lambda: retrieval_measure_ragged(f1.view(-1, C), off, f2.view(-1, C), off), a.warmup, a.steps)
    flop = 2.0 * C * S * S * N * N
    print(f"retrieval 16 x 16 shapes of {N} points: fixed-length {ms_fixed:7.3f} ms ({flop / ms_fixed / 1e9:6.1f} TFLOP/s), "
          f"ragged {ms_rag:7.3f} ms ({flop / ms_rag / 1e9:6.1f} TFLOP/s) = {ms_rag / ms_fixed:4.2f}x the fixed-length time", flush=True)
    rng = np.random.default_rng(2)
    n1, n2 = rng.integers(1000, 5001, S).tolist(), rng.integers(1000, 5001, S).tolist()
    r1 = torch.randn((sum(n1), C), device="cuda", generator=g)
    r2 = torch.randn((sum(n2), C), device="cuda", generator=g)
    o1 = np.concatenate([[0], np.cumsum(n1)]).tolist()
    o2 = np.concatenate([[0], np.cumsum(n2)]).tolist()
    ms = timed(lambda: retrieval_measure_ragged(r1, o1, r2, o2), a.warmup, a.steps)
    flop = 2.0 * C * sum(n1) * sum(n2)
    print(f"retrieval ragged 16 x 16 shapes of 1000..5000 points: {ms:7.3f} ms, {flop / ms / 1e9:6.1f} TFLOP/s over real point "
          f"pairs = {flop / ms / 1e9 / 157.3:.3f} of the fp32 matrix peak", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=8)
    ap.add_argument("--ks", default="1,3")
    ap.add_argument("--modes", default="1,0")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-loop", action="store_true", help="time only SimCSNHead (e.g. under a profiler)")
    ap.add_argument("--no-retrieval", action="store_true")
    ap.add_argument("--points", default="3000,5000", help="LO,HI: points per shape of the head benchmark")
    ap.add_argument("--flows", default="", help="comma list of kept / free / auto: time these data flows of SimCSNHead, alternating")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of --flows")
    ap.add_argument("--loss", default="", help="comma list of torch / fused: time the head's train step under these losses, alternating")
    a = ap.parse_args()
    for mode in (int(m) for m in a.modes.split(",")):
        for K in (int(k) for k in a.ks.split(",")):
            bench_head(a, mode, K)
    if a.loss:
        bench_evaluate(a)
    if not a.no_retrieval and not a.flows and not a.loss:
        bench_retrieval(a)
    _lib.lib().csn_set_math_mode(1)


if __name__ == "__main__":
    main()
