"""Float64 restatements of the ragged cross-shape head kernels (csn_amd/csrc/minkowski_csn.hip; include/csn_hip.h section 11), as
the header of the kernel file states them, with the scales the bounds of tests/test_gpu_ragged_head.py are computed from:

  pool      pooled[e][c] = gamma[c] mean_{n < counts[e]} xhat[e][c][n] + beta[c]
  pool bwd  dxhat[e][c][n] = prev + (n < counts[e] ? gamma[c] dpooled[e][c] / counts[e] : 0), n < ld
  mix fwd   out[off[b] + n][c] = sum_j comp[b][j] (gamma[c] xhat[ev(b,j)][c][n] + beta[c]), n < the shape's points
  mix bwd   dxhat[ev(b,j)][c][n] = comp[b][j] gamma[c] dout[off[b] + n][c] (0 from the shape's points to ld);
            rowdot[b][j][c] = sum_n dout xhat[ev(b,j)], rowsum[b][c] = sum_n dout; d comp, d gamma, d beta follow from them
  ev(b, 0) = b,  ev(b, j > 0) = cross_first + (j - 1) n_shapes + b

Beside a value, the same expression with the absolute value of every term (``A`` of the mix forward, sum |d x| of rowdot, sum |d| of
rowsum).  The forwards are plain differentiable torch, so tests/test_cpu_ragged_head.py holds every closed-form backward here to
autograd of the forward beside it, and ``head`` (the whole ``_RaggedHead`` node) is differentiated by autograd alone.

The case tables of the GPU module live here too, so that the CPU module can assert what they are named for."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                     # unit roundoff of fp32
CANARY = -777.25
POISON = 1e30                      # finite: the mix backward forms 0 * xhat past a shape's points (kernel file header)

# pool: counts on either side of the 4-point vector, of a wave's and the work-group's first pass (256 / 1024 points) and of the
# 1024-point stride of the pool loop and of the pool-backward grid; ld the longest count, then one with points (and a grid block)
# past every count
POOL_COUNTS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028]
POOL_LDS = (1028, 2052)
POOL_CS = (1, 5, 64)
POOL_SUB = (3, 5)                  # (first, n): the sub-range call of ``_RaggedHead.backward``

# mix: lengths on either side of the 64-point tile, the last shape shorter than a tile; ld that ends inside the longest shape's
# last tile (132), at its end (192) and a whole tile and a part of one past it (260: five tiles, the longest shape has three).
# One shape alone: the last shape is also the first
MIX_LENS = ([1, 63, 64, 65, 129, 4], [130])
MIX_LDS = (132, 192, 260)
MIX_CS = (4, 60, 64, 68, 256)
MIX_PAD = 3                        # the evaluation stride is C ld + 4 MIX_PAD


def mix_layouts(B):
    """(k1, cross_first): k1 = 1 (cross_first is not used: anything), one neighbour right behind the shapes, the head's own layout
    (S, then T, then the cross evaluations) and k1 = 8 with three unmixed evaluations in between."""
    return [(1, 7), (2, B), (3, 3 * B), (8, B + 3)]


def mix_n_evals(B, k1, cross_first):
    """Two more evaluations than the last mixed one."""
    return (B if k1 == 1 else cross_first + (k1 - 1) * B) + 2


# the node: B = 3, key batch i holds the i-th neighbour of every query shape
NODE_C = 128
NODE_LENS = [5, 65, 130]
NODE_KEY_LENS = [[3, 64, 131], [129, 7, 66], [1, 130, 4]]
NODE_CASES = [(0, False), (0, True), (1, False), (3, False)]          # (K, ssa_only)


def ev(b, j, n_shapes, cross_first):
    return b if j == 0 else cross_first + (j - 1) * n_shapes + b


def offsets(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


def _randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def make_maps(rng, counts, C, ld, pad=0):
    """xhat as (E, C, ld) inside a flat float32 buffer of evaluation stride C ld + 4 pad: (buffer, stride).  The points
    [counts[e], ld) of every row hold +-POISON alternating, the stride padding holds CANARY."""
    E, stride = len(counts), C * ld + 4 * pad
    buf = torch.full((E * stride,), CANARY, dtype=torch.float32)
    x = maps(buf, E, C, ld, stride)
    x.copy_(_randn(rng, E, C, ld))
    sign = torch.where(torch.arange(ld) % 2 == 0, POISON, -POISON).float()
    for e, n in enumerate(counts):
        x[e, :, n:] = sign[n:]
    return buf, stride


def maps(buf, E, C, ld, stride):
    """The (E, C, ld) view of a flat buffer of evaluation stride ``stride`` (the buffer may be longer: a guard behind it)."""
    return torch.as_strided(buf, (E, C, ld), (stride, ld, 1))


def padding(buf, E, C, ld, stride):
    """The (E, stride - C ld) view of the stride padding."""
    return torch.as_strided(buf, (E, stride - C * ld), (stride, 1), C * ld)


def mix_counts(lens, k1, cross_first, n_evals):
    """Point counts of the evaluations of one mix: the shape's length where (b, j) maps, and 2 where nothing does."""
    B = len(lens)
    counts = [2] * n_evals
    for b in range(B):
        for j in range(k1):
            counts[ev(b, j, B, cross_first)] = lens[b]
    return counts


def mix_inputs(lens, k1, cross_first, C, ld, pad=MIX_PAD, seed=0):
    """fp32 inputs of one mix case: the maps (``make_maps``), comp (B, k1) with |comp| <= 2 and both signs, gamma, beta,
    dout (N, C), and ``wide`` (N, 2C + 4): the real values around dout where it is a column slice of wider rows."""
    B, N = len(lens), sum(lens)
    n_evals = mix_n_evals(B, k1, cross_first)
    rng = np.random.default_rng(5000 + 1000 * seed + 131 * B + 17 * k1 + 7 * C + ld + cross_first)
    counts = mix_counts(lens, k1, cross_first, n_evals)
    buf, stride = make_maps(rng, counts, C, ld, pad)
    comp = _randn(rng, B, k1).clamp(-2.0, 2.0)
    return {"buf": buf, "stride": stride, "n_evals": n_evals, "counts": counts, "comp": comp, "gamma": _randn(rng, C),
            "beta": _randn(rng, C), "dout": _randn(rng, N, C), "wide": _randn(rng, N, 2 * C + 4)}


def pool_inputs(C, ld, pad, counts=POOL_COUNTS, seed=0):
    """fp32 inputs of one pool case: the maps, gamma, beta, dpooled (E, C) and the previous content of dxhat (a buffer laid out as
    the maps, CANARY in its stride padding)."""
    E = len(counts)
    rng = np.random.default_rng(9000 + 1000 * seed + 7 * C + ld + pad)
    buf, stride = make_maps(rng, counts, C, ld, pad)
    prev = torch.full((E * stride,), CANARY, dtype=torch.float32)
    maps(prev, E, C, ld, stride).copy_(_randn(rng, E, C, ld))
    return {"buf": buf, "stride": stride, "gamma": _randn(rng, C), "beta": _randn(rng, C), "dpooled": _randn(rng, E, C), "prev": prev}


# ------------------------------------------------------------------------------------------------------
# pool
# ------------------------------------------------------------------------------------------------------
def pool(xhat, counts, gamma, beta):
    """(pooled, mean, scale), each (E, C): scale = |gamma| mean |xhat| + |beta|."""
    gamma, beta = gamma.double(), beta.double()
    mean, mabs = [], []
    for e, n in enumerate(counts):
        x = xhat[e, :, :n].double()
        mean.append(x.sum(dim=1) / n)
        mabs.append(x.abs().sum(dim=1) / n)
    mean, mabs = torch.stack(mean), torch.stack(mabs)
    return gamma * mean + beta, mean, gamma.abs() * mabs + beta.abs()


def pool_bwd(dpooled, gamma, counts, ld, prev=None):
    """(dxhat (E, C, ld), g (E, C)): g = gamma dpooled / count is what every point below the count receives; ``prev`` (E, C, ld)
    is what the map held (accumulate = 1), None: zeros."""
    E, C = dpooled.shape
    g = gamma.double() * dpooled.double() / torch.tensor(counts, dtype=torch.float64)[:, None]
    dx = torch.zeros(E, C, ld, dtype=torch.float64) if prev is None else prev.double().clone()
    for e, n in enumerate(counts):
        dx[e, :, :n] += g[e][:, None]
    return dx, g


def pool_param_grads(dpooled, mean):
    """(dgamma, dbeta) of the pool: sum_e dpooled mean, sum_e dpooled."""
    return (dpooled.double() * mean.double()).sum(dim=0), dpooled.double().sum(dim=0)


# ------------------------------------------------------------------------------------------------------
# mix
# ------------------------------------------------------------------------------------------------------
def mix_fwd(xhat, lens, comp, gamma, beta, cross_first):
    """(out, A), each (N, C) point-major: A = |gamma| sum_j |comp_j xhat_j| + |beta| sum_j |comp_j|."""
    comp, gamma, beta = comp.double(), gamma.double(), beta.double()
    B, k1 = comp.shape
    out, scale = [], []
    for b, n in enumerate(lens):
        terms = torch.stack([comp[b, j] * xhat[ev(b, j, B, cross_first), :, :n].double() for j in range(k1)])      # (k1, C, n)
        val = gamma[:, None] * terms.sum(dim=0) + beta[:, None] * comp[b].sum()
        a = gamma.abs()[:, None] * terms.abs().sum(dim=0) + beta.abs()[:, None] * comp[b].abs().sum()
        out.append(val.t())
        scale.append(a.t())
    return torch.cat(out), torch.cat(scale)


def mix_bwd(dout, xhat, lens, comp, gamma, cross_first):
    """dxhat (E, C, ld; zero wherever nothing maps), written (E,) bool: the evaluations some (b, j) maps to, rowdot (B, k1, C),
    rowsum (B, C) and the scales dot_abs = sum_n |dout xhat|, sum_abs = sum_n |dout|."""
    dout, comp, gamma = dout.double(), comp.double(), gamma.double()
    B, k1 = comp.shape
    E, C, ld = xhat.shape
    off = offsets(lens)
    dx = torch.zeros(E, C, ld, dtype=torch.float64)
    written = torch.zeros(E, dtype=torch.bool)
    rowdot, dot_abs = torch.zeros(B, k1, C, dtype=torch.float64), torch.zeros(B, k1, C, dtype=torch.float64)
    rowsum, sum_abs = torch.zeros(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64)
    for b, n in enumerate(lens):
        d = dout[off[b]:off[b + 1]].t()                                # (C, n)
        rowsum[b], sum_abs[b] = d.sum(dim=1), d.abs().sum(dim=1)
        for j in range(k1):
            e = ev(b, j, B, cross_first)
            dx[e, :, :n] = comp[b, j] * gamma[:, None] * d
            written[e] = True
            prod = d * xhat[e, :, :n].double()
            rowdot[b, j], dot_abs[b, j] = prod.sum(dim=1), prod.abs().sum(dim=1)
    return {"dxhat": dx, "written": written, "rowdot": rowdot, "rowsum": rowsum, "dot_abs": dot_abs, "sum_abs": sum_abs}


def mix_param_grads(rowdot, rowsum, comp, gamma, beta):
    """(dcomp (B, k1), dgamma (C,), dbeta (C,)) from the reductions:
    dcomp[b][j] = sum_c rowdot[b][j][c] gamma[c] + sum_c rowsum[b][c] beta[c];  dgamma[c] = sum_{b,j} comp[b][j] rowdot[b][j][c];
    dbeta[c] = sum_b (sum_j comp[b][j]) rowsum[b][c]."""
    rowdot, rowsum, comp, gamma, beta = (t.double() for t in (rowdot, rowsum, comp, gamma, beta))
    dcomp = (rowdot * gamma).sum(dim=2) + (rowsum * beta).sum(dim=1, keepdim=True)
    dgamma = (comp[:, :, None] * rowdot).sum(dim=(0, 1))
    dbeta = (comp.sum(dim=1, keepdim=True) * rowsum).sum(dim=0)
    return dcomp, dgamma, dbeta


# ------------------------------------------------------------------------------------------------------
# the node: pool, linear_q / linear_k, normalize, sim, softmax, mix
# ------------------------------------------------------------------------------------------------------
def node_counts(lens, key_lens, K):
    """Point counts in the evaluation order of ``SimCSNHead.forward``: S_b, T_{i,b}, X_{i,b}."""
    return list(lens) + [n for ks in key_lens[:K] for n in ks] + list(lens) * K


def node_inputs(K, seed=0):
    """fp32 inputs of one node case: the maps (ld = round-up-4 of the longest count, no stride padding: the node takes a dense
    tensor), gamma, beta, wq, wk (C, C) of variance 1 / C, q_rows (N, C) and the upstream gradient (N, 2C)."""
    C, N = NODE_C, sum(NODE_LENS)
    counts = node_counts(NODE_LENS, NODE_KEY_LENS, K)
    ld = (max(counts) + 3) // 4 * 4
    rng = np.random.default_rng(12000 + 1000 * seed + K)
    buf, stride = make_maps(rng, counts, C, ld)
    return {"xhat": maps(buf, len(counts), C, ld, stride), "counts": counts, "gamma": 1.0 + 0.1 * _randn(rng, C), "beta": 0.1 * _randn(rng, C),
            "wq": _randn(rng, C, C) / C ** 0.5, "wk": _randn(rng, C, C) / C ** 0.5, "q_rows": _randn(rng, N, C), "dout": _randn(rng, N, 2 * C)}


def head(xhat, q_rows, lens, counts, K, ssa_only, gamma, beta, wq, wk, temperature):
    """The ``_RaggedHead`` node from the restatements above (hrnet.py:366-411): (N, 2C) = [q | csa], or the SSA rows (N, C).  All
    tensors float64; differentiable."""
    B = len(lens)
    if K > 0 and not ssa_only:
        n_pool = B * (K + 1)
        pooled = pool(xhat, counts[:n_pool], gamma, beta)[0]
        p = pooled.view(K + 1, B, -1).transpose(0, 1)                  # (B, K+1, C), slot 0 = S_b
        u = F.normalize(F.linear(p[:, 0], wq), dim=-1)
        w = F.normalize(F.linear(p, wk), dim=-1)
        sim = torch.bmm(u.unsqueeze(1), w.transpose(1, 2)).squeeze(1) / temperature
        comp = F.softmax(sim, dim=-1)
    else:
        comp = torch.ones(B, 1, dtype=torch.float64)
    csa = mix_fwd(xhat, lens, comp, gamma, beta, B + K * B)[0]
    return csa if ssa_only else torch.cat([q_rows, csa], dim=1)
