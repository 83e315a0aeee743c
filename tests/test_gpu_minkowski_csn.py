"""GPU parity of the MinkowskiNet cross-shape head on ragged shape batches (csn_amd/minkowski_csn.py): the head against a float64
restatement of hrnet.py:359-423 written on top of oracle.mha_pointmajor, against the existing layer called per shape, in train
mode, the ragged retrieval measure against float64 and against the fixed-length kernel, and the shape graph of
csn_utils.py:44-97 against its float64 restatement — in both math modes."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(autouse=True, params=[0, 1], ids=["fp32", "bf16x3"])
def math_mode(request, L):
    L.check(L.lib().csn_set_math_mode(request.param))
    yield request.param
    L.lib().csn_set_math_mode(1)


# ------------------------------------------------------------------------------------------------------
# float64 restatement of the head (hrnet.py:359-423) and of cosine_similarity (:472-490)
# ------------------------------------------------------------------------------------------------------
def _mha64(a, b, p, H, d):
    from oracle import csa_oracle as orc
    return orc.mha_pointmajor(a[None], b[None], b[None], p, H, d, d, prefix="MHA.")[0][0]


def ref_head(qs, keys, p, H, C, return_ssa=False):
    """qs: per-shape (n_b, C) rows; keys: K lists of per-shape rows; p: float64 parameters named as SimCSNHead's."""
    d = C // H
    ssa = [_mha64(q, q, p, H, d) for q in qs]                                                   # get_SSA, :456-470
    if return_ssa:
        return torch.cat(ssa)
    K = len(keys)
    if K == 0:
        csa = ssa
    else:
        csa = []
        for b, q in enumerate(qs):
            u = F.normalize(ssa[b].mean(0) @ p["linear_q.weight"].t(), dim=-1)               # :380-383
            slots = [ssa[b]] + [_mha64(keys[i][b], keys[i][b], p, H, d) for i in range(K)]
            sims = [(u * F.normalize(t.mean(0) @ p["linear_k.weight"].t(), dim=-1)).sum() / C ** 0.5 for t in slots]
            comp = torch.softmax(torch.stack(sims), dim=0)                                     # :397
            out = comp[0] * ssa[b]
            for i in range(K):
                out = out + comp[i + 1] * _mha64(q, keys[i][b], p, H, d)                        # :400-411
            csa.append(out)
    x = torch.cat([torch.cat(qs), torch.cat(csa)], dim=1)                                       # :423
    return x @ p["output.weight"].t() + p["output.bias"]


def ref_cosine(q, k):
    """hrnet.py:472-490 in float64 (the rows here are never all-zero, so the 1e-12 clamp of the kernels does not matter)."""
    qn = q / (q ** 2).sum(1, keepdim=True).sqrt()
    kn = k / (k ** 2).sum(1, keepdim=True).sqrt()
    return (qn @ kn.t()).max(1).values.mean()


# ------------------------------------------------------------------------------------------------------
def _params(rng, H, C, out_ch, K):
    """Head parameters with the out-projection scaled up as in oracle.conditioned_csa_case (fc x 4), so that the K+1 maps
    differ materially.  (w_qs is left unscaled: sharper attention only inflates the bf16x3 error of the layer's own
    W_q / W_k gradients, which test_gpu_minkowski.py already covers.)"""
    from oracle import csa_oracle as orc
    d = C // H
    a = orc.make_params(rng, H, d_model=C, d_k=d, d_v=d)
    p = {"MHA." + k[len("attention."):]: v for k, v in a.items() if k.startswith("attention.")}
    p["MHA.fc.weight"] = p["MHA.fc.weight"] * 4.0
    p["MHA.norm.weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32))
    p["MHA.norm.bias"] = torch.from_numpy(rng.uniform(-0.3, 0.3, C).astype(np.float32))
    u = lambda shape, bound: torch.from_numpy(rng.uniform(-bound, bound, shape).astype(np.float32))
    p["output.weight"] = u((out_ch, 2 * C), 1 / math.sqrt(2 * C))
    p["output.bias"] = u((out_ch,), 1 / math.sqrt(2 * C))
    if K > 0:
        p["linear_q.weight"] = u((C, C), 1 / math.sqrt(C)) * 3.0
        p["linear_k.weight"] = u((C, C), 1 / math.sqrt(C)) * 3.0
    return p


def _shape(rng, n, C):
    """a shape's rows with its own channel offset (constant along the points): pooled descriptors and comp differ per shape"""
    return torch.from_numpy((rng.standard_normal((n, C)) + 0.8 * rng.standard_normal((1, C))).astype(np.float32))


def _head(p, C, H, out_ch, K, dropout=0.1):
    from csn_amd.minkowski_csn import SimCSNHead
    h = SimCSNHead(C, H, out_ch, K, dropout=dropout)
    h.load_state_dict(p)
    return h.cuda()


def _pack(shapes):
    off = [0]
    for s in shapes:
        off.append(off[-1] + s.shape[0])
    return torch.cat(shapes), off


def _rel(got, want):
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


CASES = [  # (q lengths, key lengths per neighbour rank, n_head, d_model)
    ([301], [], 4, 256),
    ([5, 37, 7], [[301, 1, 5]], 4, 256),
    ([7, 1301, 5], [[37, 5, 1], [1, 301, 7], [5, 7, 37]], 3, 256),
    ([37], [[5], [301], [1]], 4, 128),
    ([1, 5, 301], [], 4, 128),
]


@pytest.mark.parametrize("qlens,klens,H,C", CASES, ids=[f"B{len(c[0])}K{len(c[1])}H{c[2]}C{c[3]}" for c in CASES])
def test_head_against_float64(L, math_mode, qlens, klens, H, C):
    """Outputs within 1e-4 absolute, gradients to the query rows, every key batch and every parameter within 1e-4 of each
    tensor's max.  Measured on MI355X: outputs <= 9e-7 (fp32) / 6e-6 (bf16x3), gradients <= 5e-6 (fp32) / 2.5e-5 (bf16x3),
    linear_q / linear_k <= 8e-7 (fp32) / 1.8e-5 (bf16x3): the per-shape offsets make them well-conditioned."""
    rng = np.random.default_rng(41 + len(qlens) + 7 * len(klens) + H)
    K, out_ch = len(klens), 11
    p = _params(rng, H, C, out_ch, K)
    qs = [_shape(rng, n, C) for n in qlens]
    keys = [[_shape(rng, m, C) for m in ms] for ms in klens]
    g = torch.from_numpy(rng.standard_normal((sum(qlens), out_ch)).astype(np.float32))

    head = _head(p, C, H, out_ch, K).eval()
    q, qo = _pack(qs)
    qd = q.cuda().requires_grad_(True)
    kd = [(_pack(ks)[0].cuda().requires_grad_(True), _pack(ks)[1]) for ks in keys]
    out = head(qd, qo, kd if K else None)
    assert out.shape == (sum(qlens), out_ch)
    (out * g.cuda()).sum().backward()

    p64 = {n: t.double().requires_grad_(True) for n, t in p.items()}
    q64 = [t.double().requires_grad_(True) for t in qs]
    k64 = [[t.double().requires_grad_(True) for t in ks] for ks in keys]
    ref = ref_head(q64, k64, p64, H, C)
    (ref * g.double()).sum().backward()

    e_out = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    e = {"dq": _rel(qd.grad, torch.cat([t.grad for t in q64]))}
    for i, ks in enumerate(k64):
        e[f"dk{i}"] = _rel(kd[i][0].grad, torch.cat([t.grad for t in ks]))
    for name, prm in head.named_parameters():
        e[name] = _rel(prm.grad, p64[name].grad)
    print(f"[minkowski_csn] mode {math_mode} q {qlens} k {klens} H={H} C={C}: out {e_out:.1e} "
          + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
    assert e_out < 1e-4
    assert max(e.values()) < 1e-4, e


def test_head_against_the_layer_per_shape(L, math_mode):
    """Eval mode: return_ssa and the K = 0 head equal per-shape calls of the existing MultiHeadAttention; the full head equals
    the same composition done per shape with torch head math (fp32: 1e-5; bf16x3: 1e-4, the padded batch takes other GEMM
    tilings)."""
    tol = 1e-5 if math_mode == 0 else 1e-4
    rng = np.random.default_rng(7)
    H, C, K, out_ch = 4, 256, 2, 9
    p = _params(rng, H, C, out_ch, K)
    qlens, klens = [5, 130, 37], [[7, 1, 301], [64, 5, 9]]
    qs = [_shape(rng, n, C).cuda() for n in qlens]
    keys = [[_shape(rng, m, C).cuda() for m in ms] for ms in klens]
    head = _head(p, C, H, out_ch, K).eval()
    q, qo = _pack(qs)
    with torch.no_grad():
        ssa = head(q, qo, return_ssa=True)
        per = [head.MHA(t[None], t[None], t[None])[0][0] for t in qs]
        assert (ssa - torch.cat(per)).abs().max().item() < tol
        head0 = _head({k: v for k, v in p.items() if not k.startswith("linear_")}, C, H, out_ch, 0).eval()
        out0 = head0(q, qo)
        want0 = F.linear(torch.cat([q, torch.cat(per)], 1), head0.output.weight, head0.output.bias)
        assert (out0 - want0).abs().max().item() < tol
        out = head(q, qo, [_pack(ks) for ks in keys])
        csa = []
        for b, t in enumerate(qs):
            s = per[b]
            u = F.normalize(head.linear_q(s.mean(0)), dim=-1)
            slots = [s] + [head.MHA(keys[i][b][None], keys[i][b][None], keys[i][b][None])[0][0] for i in range(K)]
            sims = torch.stack([head.sim(u[None], F.normalize(head.linear_k(x.mean(0)), dim=-1)[None]).squeeze() for x in slots])
            comp = torch.softmax(sims, 0)
            c = comp[0] * s
            for i in range(K):
                c = c + comp[i + 1] * head.MHA(t[None], keys[i][b][None], keys[i][b][None])[0][0]
            csa.append(c)
        want = head.output(torch.cat([q, torch.cat(csa)], 1))
        assert (out - want).abs().max().item() < tol


def test_train_mode(L, math_mode):
    """Dropout live: outputs differ from eval, outputs and gradients finite; with both dropout p = 0 train equals eval bitwise."""
    rng = np.random.default_rng(9)
    H, C, K, out_ch = 4, 128, 2, 6
    p = _params(rng, H, C, out_ch, K)
    qs = [_shape(rng, n, C) for n in (5, 90, 33)]
    keys = [[_shape(rng, m, C) for m in ms] for ms in ([17, 3, 64], [8, 51, 1])]
    q, qo = _pack(qs)
    kb = [(_pack(ks)[0].cuda(), _pack(ks)[1]) for ks in keys]
    head = _head(p, C, H, out_ch, K)
    with torch.no_grad():
        ev = head.eval()(q.cuda(), qo, kb)
    head.train()
    torch.manual_seed(3)
    qd = q.cuda().requires_grad_(True)
    tr = head(qd, qo, kb)
    tr.square().sum().backward()
    assert torch.isfinite(tr).all() and (tr - ev).abs().max().item() > 1e-3
    assert torch.isfinite(qd.grad).all() and all(torch.isfinite(prm.grad).all() for prm in head.parameters())
    head.MHA.dropout.p = 0.0
    head.MHA.attention.dropout.p = 0.0
    with torch.no_grad():
        tr0 = head.train()(q.cuda(), qo, kb)
        ev0 = head.eval()(q.cuda(), qo, kb)
    assert torch.equal(tr0, ev0) and torch.equal(ev0, ev)


def test_ragged_retrieval_against_float64(L, math_mode):
    """5 x 7 shapes of 1 .. 5000 points (127 / 128 / 129 included); key 6 is the NEGATION of query 3, so every one of its
    cosines is <= 0 — a zero-padded candidate (cos = 0) would win the max there."""
    from csn_amd.minkowski_csn import retrieval_measure_ragged, cosine_similarity
    rng = np.random.default_rng(13)
    C = 256
    ql, kl = [1, 127, 128, 129, 700], [5000, 129, 1, 128, 37, 127]
    qs = [_shape(rng, n, C).cuda() for n in ql]
    ks = [_shape(rng, n, C).cuda() for n in kl] + [-qs[3]]
    f1, o1 = _pack(qs)
    f2, o2 = _pack(ks)
    got = retrieval_measure_ragged(f1, o1, f2, o2)
    want = torch.stack([torch.stack([ref_cosine(a.double(), b.double()) for b in ks]) for a in qs]).cpu()
    assert want[3, 6] < 0
    err = (got.cpu().double() - want).abs().max().item()
    assert err < 1e-5, err
    assert abs(cosine_similarity(qs[4], ks[0]).item() - want[4, 0].item()) < 1e-5
    assert torch.equal(retrieval_measure_ragged(f1, o1, f2, o2), got)                  # fixed order: bitwise reproducible


def test_ragged_retrieval_equals_fixed_length_kernel(L, math_mode):
    from csn_amd import functional as CF
    from csn_amd.minkowski_csn import retrieval_measure_ragged
    rng = np.random.default_rng(14)
    S1, S2, N, C = 3, 4, 300, 128
    a = torch.from_numpy(rng.standard_normal((S1, N, C)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal((S2, N, C)).astype(np.float32)).cuda()
    fixed = CF.retrieval_measure(a, b)
    ragged = retrieval_measure_ragged(a.reshape(-1, C), [i * N for i in range(S1 + 1)], b.reshape(-1, C),
                                      [i * N for i in range(S2 + 1)])
    assert (fixed - ragged).abs().max().item() < 1e-6


def _clustered(rng, S, lens, C, n_centers=3):
    """ragged shapes around a few shared channel offsets, each shape with its own smaller offset (a tie-free ranking)"""
    centers = rng.standard_normal((n_centers, 1, C)) * 2.0
    return [torch.from_numpy((centers[s % n_centers] + 0.8 * rng.standard_normal((1, C)) + rng.standard_normal((n, C)))
                             .astype(np.float32)) for s, n in zip(range(S), lens)]


def _ref_graph(shapes_q, shapes_k, p, H, C, K):
    """csn_utils.py:44-97 restated in float64: the SSA of every shape, cosine_similarity of every pair, the top-K rule."""
    d = C // H
    with torch.no_grad():
        sq = [_mha64(t.double(), t.double(), p, H, d) for t in shapes_q]
        sk = sq if shapes_k is None else [_mha64(t.double(), t.double(), p, H, d) for t in shapes_k]
        sim = torch.stack([torch.stack([ref_cosine(a, b) for b in sk]) for a in sq])
    out = []
    for q in range(len(sq)):
        _, idx = torch.topk(sim[q], K)
        if shapes_k is None and q in idx:
            _, idx = torch.topk(sim[q], K + 1)
            idx = idx[q != idx]
        out.append((q, idx.tolist()))
    return out, sim


def test_shape_graph_against_float64(L, math_mode):
    from csn_amd.minkowski_csn import construct_shape_graph
    rng = np.random.default_rng(23)
    H, C, K = 4, 128, 2
    p = _params(rng, H, C, 5, K)
    p64 = {n: t.double() for n, t in p.items()}
    qsh = _clustered(rng, 7, [40, 75, 130, 33, 90, 5, 57], C)
    ksh = _clustered(rng, 5, [61, 9, 120, 44, 101], C)
    head = _head(p, C, H, 5, K).eval()
    for keys in (None, ksh):
        want, sim = _ref_graph(qsh, keys, p64, H, C, K)
        # the case is tie-free: the ranking is decided by gaps far above fp32 rounding
        srt = sim.sort(dim=1, descending=True).values
        assert (srt[:, :K + 1] - srt[:, 1:K + 2]).min().item() > 1e-4
        got = construct_shape_graph(head, [t.cuda() for t in qsh], None if keys is None else [t.cuda() for t in keys], K=K,
                                    max_rows=200)
        assert got == want, (got, want)
