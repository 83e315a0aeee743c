"""The score-free backward of the MinkowskiNet attention at module level (csn_amd.tuning.cross_score_free / cross_score_budget):
MultiHeadAttention.forward, forward_varlen and SimCSNHead under ``tuning.override(cross_score_free=True)`` against the float64
restatements of tests/test_gpu_minkowski.py and tests/test_gpu_minkowski_csn.py at their 1e-4; train mode against the kept flow
under the same seeds; which entry points each setting of the switches takes; and the memory condition the flow exists for:
one forward + backward at 6000 x 6000 points allocates less than ONE score tensor, where the kept flow holds three."""
import gc

import numpy as np
import pytest
import torch

import tests.test_gpu_minkowski as tm
import tests.test_gpu_minkowski_csn as tc

pytestmark = pytest.mark.gpu

FLASH = ("csn_cross_attn_bwd_flash_f32", "csn_varlen_attn_bwd_flash_f32")
KEPT = ("csn_cross_attn_bwd_f32", "csn_varlen_attn_bwd_f32")


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _mode(L):
    L.check(L.lib().csn_set_math_mode(1))
    yield
    L.set_call_hook(None)
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


class Calls:
    """the entry points a block launches, recorded through csn_amd._lib.set_call_hook"""

    def __init__(self, L):
        self.L, self.names = L, []

    def __enter__(self):
        self.L.set_call_hook(lambda name, phase: self.names.append(name) if phase == "begin" else None)
        return self

    def __exit__(self, *exc):
        self.L.set_call_hook(None)

    def backward_flows(self):
        return [n for n in self.names if n in FLASH + KEPT]


def _rel(got, want):
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("b,lq,lk,H,C", [(2, 7, 301, 4, 256), (1, 37, 1301, 4, 256), (1, 1301, 37, 4, 256), (2, 301, 7, 4, 256),
                                         (1, 301, 1301, 4, 128), (2, 37, 301, 1, 128), (1, 301, 37, 1, 96), (1, 90, 61, 5, 256)])
def test_forward_backward_against_float64(L, b, lq, lk, H, C):
    """MultiHeadAttention.forward, eval mode, d_head = 64, 32, 128, 96 and 51 (run at 64): outputs, attn and every gradient"""
    from csn_amd import tuning
    from oracle import csa_oracle as orc
    rng = np.random.default_rng(117)
    d = C // H
    p = tm._params(rng, H, C, d)
    m = tm._module(p, H, C, d).eval()
    q, k, v = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((b, lq, C), (b, lk, C), (b, lk, C)))
    g = torch.from_numpy(rng.standard_normal((b, lq, C)).astype(np.float32))
    qd, kd, vd = (t.cuda().requires_grad_(True) for t in (q, k, v))
    with tuning.override(cross_score_free=True), Calls(L) as calls:
        out, attn = m(qd, kd, vd)                                          # (return_attention: scores exist for attn, unsaved)
        out.backward(g.cuda())
    assert calls.backward_flows() == [FLASH[0]]
    p64 = {n: t.double().requires_grad_(True) for n, t in p.items() if n.startswith("attention.")}
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ref, rattn = orc.mha_pointmajor(q64, k64, v64, p64, H, d, d)
    ref.backward(g.double())
    e_out = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    e_attn = (attn.cpu().double() - rattn.detach()).abs().max().item()
    e = {n: _rel(a.grad, r.grad) for n, a, r in (("dq", qd, q64), ("dk", kd, k64), ("dv", vd, v64))}
    e.update({name: _rel(prm.grad, p64["attention." + name].grad) for name, prm in m.named_parameters()})
    print(f"[score-free] b={b} lq={lq} lk={lk} H={H} C={C}: out {e_out:.1e} attn {e_attn:.1e} " + " ".join(f"{n} {x:.1e}" for n, x in e.items()))
    assert e_out < 1e-4 and e_attn < 1e-4
    assert max(e.values()) < 1e-4, e


LENS = [(7, 301), (45, 70), (1301, 37), (512, 500), (100, 1), (37, 1301)]


def _ragged_case(rng, C):
    qs = [torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)) for n, _ in LENS]
    ks = [torch.from_numpy(rng.standard_normal((m, C)).astype(np.float32)) for _, m in LENS]
    vs = [torch.from_numpy(rng.standard_normal((m, C)).astype(np.float32)) for _, m in LENS]
    gs = [torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)) for n, _ in LENS]
    return qs, ks, vs, gs


def test_forward_varlen_against_float64(L):
    """forward_varlen, eval mode: every pair's output and the gradients to every input and weight against the float64 oracle
    called pair by pair"""
    from csn_amd import tuning
    from oracle import csa_oracle as orc
    rng = np.random.default_rng(129)
    H, C = 4, 256
    d = C // H
    p = tm._params(rng, H, C, d)
    qs, ks, vs, gs = _ragged_case(rng, C)
    m = tm._module(p, H, C, d).eval()
    qd, kd, vd = ([t.cuda().requires_grad_(True) for t in ts] for ts in (qs, ks, vs))
    with tuning.override(cross_score_free=True), Calls(L) as calls:
        outs = m.forward_varlen(qd, kd, vd)
        sum((o * g.cuda()).sum() for o, g in zip(outs, gs)).backward()
    assert calls.backward_flows() == [FLASH[1]]
    p64 = {n: t.double().requires_grad_(True) for n, t in p.items() if n.startswith("attention.")}
    q64, k64, v64 = ([t.double().requires_grad_(True) for t in ts] for ts in (qs, ks, vs))
    total = 0
    for i in range(len(LENS)):
        ref, _ = orc.mha_pointmajor(q64[i][None], k64[i][None], v64[i][None], p64, H, d, d)
        assert (outs[i].detach().cpu().double() - ref[0].detach()).abs().max().item() < 1e-4, i
        total = total + (ref[0] * gs[i].double()).sum()
    total.backward()
    # the rule test_gpu_minkowski.py applies to a rectangular batch — one relative error per (b, len, C) gradient tensor, i.e.
    # against the largest entry over all items of the batch — restated for the ragged batch: every pair's error against the
    # largest entry of that gradient over all pairs (the pair with ONE key has dq = dk = 0 exactly in float64)
    for role, got, want in (("dq", qd, q64), ("dk", kd, k64), ("dv", vd, v64)):
        top = max(w.grad.abs().max().item() for w in want)
        for i in range(len(LENS)):
            err = (got[i].grad.cpu().double() - want[i].grad).abs().max().item()
            assert err < 1e-4 * top, (role, i, err, top)
    for name, prm in m.named_parameters():
        assert _rel(prm.grad, p64["attention." + name].grad) < 1e-4, name


@pytest.mark.parametrize("qlens,klens,H,C", tc.CASES, ids=[f"B{len(c[0])}K{len(c[1])}H{c[2]}C{c[3]}" for c in tc.CASES])
def test_head_against_float64(L, qlens, klens, H, C):
    """SimCSNHead (K = 0, 1, 3), eval mode: the cases and the 1e-4 of tests/test_gpu_minkowski_csn.py"""
    from csn_amd import tuning
    rng = np.random.default_rng(41 + len(qlens) + 7 * len(klens) + H)
    K, out_ch = len(klens), 11
    p = tc._params(rng, H, C, out_ch, K)
    qs = [tc._shape(rng, n, C) for n in qlens]
    keys = [[tc._shape(rng, m, C) for m in ms] for ms in klens]
    g = torch.from_numpy(rng.standard_normal((sum(qlens), out_ch)).astype(np.float32))
    head = tc._head(p, C, H, out_ch, K).eval()
    q, qo = tc._pack(qs)
    qd = q.cuda().requires_grad_(True)
    kd = [(tc._pack(ks)[0].cuda().requires_grad_(True), tc._pack(ks)[1]) for ks in keys]
    with tuning.override(cross_score_free=True), Calls(L) as calls:
        out = head(qd, qo, kd if K else None)
        (out * g.cuda()).sum().backward()
    assert calls.backward_flows() == [FLASH[1]]
    p64 = {n: t.double().requires_grad_(True) for n, t in p.items()}
    q64 = [t.double().requires_grad_(True) for t in qs]
    k64 = [[t.double().requires_grad_(True) for t in ks] for ks in keys]
    ref = tc.ref_head(q64, k64, p64, H, C)
    (ref * g.double()).sum().backward()
    e_out = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    e = {"dq": _rel(qd.grad, torch.cat([t.grad for t in q64]))}
    for i, ks in enumerate(k64):
        e[f"dk{i}"] = _rel(kd[i][0].grad, torch.cat([t.grad for t in ks]))
    for name, prm in head.named_parameters():
        e[name] = _rel(prm.grad, p64[name].grad)
    print(f"[score-free head] q {qlens} k {klens} H={H} C={C}: out {e_out:.1e} " + " ".join(f"{n} {x:.1e}" for n, x in e.items()))
    assert e_out < 1e-4
    assert max(e.values()) < 1e-4, e


def _grads(ts):
    return [t.grad.detach().clone() for t in ts]


def test_train_mode_equals_the_kept_flow_under_the_same_seeds(L):
    """Dropout live (both p = 0.1): the same torch seed draws the same masks in either flow, the forward is the same launch but
    for scores = NULL — outputs bit-identical — and every gradient of the score-free flow lies within 1e-4 (of the tensor's
    max) of the kept flow's, for forward, forward_varlen and the head (K = 3)."""
    from csn_amd import tuning
    rng = np.random.default_rng(131)
    H, C = 4, 256
    d = C // H
    p = tm._params(rng, H, C, d)
    m = tm._module(p, H, C, d).train()
    q, k = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in ((2, 301, C), (2, 1301, C)))
    qs, ks, vs, gs = _ragged_case(rng, C)
    K, out_ch = 3, 11
    ph = tc._params(rng, H, C, out_ch, K)
    head = tc._head(ph, C, H, out_ch, K).train()
    hq = [tc._shape(rng, n, C) for n in (7, 1301, 37)]
    hk = [[tc._shape(rng, n, C) for n in ms] for ms in ([37, 5, 1], [1, 301, 7], [5, 7, 37])]

    def run(free):
        res = {}
        with tuning.override(cross_score_free=free), Calls(L) as calls:
            torch.manual_seed(5)
            qd, kd = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
            m.zero_grad()
            out, _ = m(qd, kd, kd)
            out.square().sum().backward()
            res["forward"] = (out.detach(), _grads([qd, kd] + list(m.parameters())))
            ql, kl, vl = ([t.cuda().requires_grad_(True) for t in ts] for ts in (qs, ks, vs))
            m.zero_grad()
            outs = m.forward_varlen(ql, kl, vl)
            sum((o * g.cuda()).sum() for o, g in zip(outs, gs)).backward()
            res["varlen"] = (torch.cat([o.detach() for o in outs]), _grads(ql + kl + vl + list(m.parameters())))
            pq, qo = tc._pack(hq)
            pqd = pq.cuda().requires_grad_(True)
            kb = [(tc._pack(x)[0].cuda().requires_grad_(True), tc._pack(x)[1]) for x in hk]
            head.zero_grad()
            o = head(pqd, qo, kb)
            o.square().sum().backward()
            res["head"] = (o.detach(), _grads([pqd] + [t for t, _ in kb] + list(head.parameters())))
        flows = calls.backward_flows()
        assert flows == ([FLASH[0], FLASH[1], FLASH[1]] if free else [KEPT[0], KEPT[1], KEPT[1]]), flows
        return res

    free, kept = run(True), run(False)
    for name in free:
        assert torch.isfinite(free[name][0]).all()
        assert torch.equal(free[name][0], kept[name][0]), f"{name}: the train-mode forward differs between the flows"
        worst = 0.0
        for a, b_ in zip(free[name][1], kept[name][1]):
            assert torch.isfinite(a).all()
            worst = max(worst, ((a - b_).abs().max() / b_.abs().max().clamp_min(1e-1)).item())
        print(f"[score-free train] {name}: worst gradient distance to the kept flow {worst:.1e}")
        assert worst < 1e-4, name


def test_selection(L):
    """cross_score_free=None: the automatic rule — a budget of one byte takes the score-free entry points, the default budget at
    a small size the kept ones; False never; True where there is no kernel raises CsnError naming mode and width."""
    from csn_amd import CsnError, tuning
    from csn_amd.minkowski_attention import MultiHeadAttention
    rng = np.random.default_rng(137)
    H, C = 4, 256
    p = tm._params(rng, H, C, C // H)
    m = tm._module(p, H, C, C // H).eval()
    qs, ks, vs, gs = _ragged_case(rng, C)

    def step(module=m, c=C):
        q = torch.randn(1, 37, c, device="cuda", requires_grad=True)
        k = torch.randn(1, 301, c, device="cuda", requires_grad=True)
        with Calls(L) as calls:
            module(q, k, k)[0].sum().backward()
            if module is m:
                ql, kl = ([t.cuda().requires_grad_(True) for t in ts] for ts in (qs, ks))
                sum(o.sum() for o in m.forward_varlen(ql, kl)).backward()
        return calls.backward_flows()

    assert step() == list(KEPT)                                                 # the default: nothing changes
    with tuning.override(cross_score_budget=1):
        assert step() == list(FLASH)
    with tuning.override(cross_score_free=None, cross_score_budget=10 ** 12):
        assert step() == list(KEPT)
    with tuning.override(cross_score_free=False, cross_score_budget=1):
        assert step() == list(KEPT)
    with tuning.override(cross_score_free=True):
        assert step() == list(FLASH)
        with torch.no_grad(), Calls(L) as calls:                               # nothing to differentiate: nothing to decide
            m(torch.randn(1, 8, C, device="cuda"), torch.randn(1, 9, C, device="cuda"), torch.randn(1, 9, C, device="cuda"))
        assert calls.backward_flows() == []
    # no kernels: exact fp32, and d_head = 256
    wide = MultiHeadAttention(1, 256, 256, 256).cuda().eval()
    with tuning.override(cross_score_budget=1):                                 # the automatic rule keeps the scores there
        assert step(wide) == [KEPT[0]]
    with tuning.override(cross_score_free=True):
        with pytest.raises(CsnError, match="256"):
            step(wide)
        L.check(L.lib().csn_set_math_mode(0))
        with pytest.raises(CsnError, match="mode 0"):
            step()
    with tuning.override(cross_score_budget=1):
        assert step() == list(KEPT)                                             # (still mode 0)


def test_peak_memory_stays_below_one_score_tensor(L):
    """The point of the flow.  One forward + backward of MultiHeadAttention(4, 256, 64, 64, return_attention=False) at b = 2,
    lq = lk = 6000: one score tensor is 2 * 4 * 6000 * 6016 * 4 B = 1.16 GB, a (b, 256, 6000) fp32 map 12.3 MB, and fewer than
    40 such maps are alive at any time (under 0.5 GB).  Score-free: the step's peak above what was allocated before it is
    below ONE score tensor.  Kept flow, same measurement: at least three (scores, the working copy, dscores)."""
    from csn_amd import tuning
    from csn_amd.minkowski_attention import MultiHeadAttention
    b, n, H, C = 2, 6000, 4, 256
    one = b * H * n * ((n + 31) // 32 * 32) * 4
    torch.manual_seed(7)
    m = MultiHeadAttention(H, C, C // H, C // H, return_attention=False).cuda().train()
    q = torch.randn(b, n, C, device="cuda", requires_grad=True)
    k = torch.randn(b, n, C, device="cuda", requires_grad=True)

    def peak(free):
        m.zero_grad(set_to_none=True)
        q.grad = k.grad = None
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with tuning.override(cross_score_free=free), Calls(L) as calls:
            out, _ = m(q, k, k)
            out.sum().backward()
            del out
        torch.cuda.synchronize()
        assert calls.backward_flows() == [FLASH[0] if free else KEPT[0]]
        assert torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all()
        return torch.cuda.max_memory_allocated() - before

    free, kept = peak(True), peak(False)
    print(f"[score-free memory] one score tensor {one / 1e9:.3f} GB; step peak: score-free {free / 1e9:.3f} GB, kept {kept / 1e9:.3f} GB")
    assert kept >= 3 * one, "the measurement does not see the kept flow's score tensors"
    assert free < one
