"""Float64 restatements of the kernels that close a cross-shape-attention step, with the scales the tests' bounds are computed
from: the compatibility-weighted mix and its reductions (csn_amd/csrc/combine.hip), the compatibility head with its backward
written out by hand (csrc/compat.hip) and the fixed-length retrieval measure (csrc/retrieval.hip).  Plain torch float64 and no
autograd in here: tests/test_cpu_tail.py holds every hand-written backward to torch autograd of the forward beside it.

The case lists of tests/test_gpu_tail.py live here too, so that tests/test_cpu_tail.py can assert on the restatements alone what
those cases rely on (a negative maximum, a finite degenerate gradient, which of C*C and B*K1*C is the larger)."""
import numpy as np
import torch

U = 2.0 ** -24                     # unit roundoff of fp32
EPS = 1e-12                        # F.normalize's clamp

# (B, K1, C, NP): NP below, at and just past one and two passes of the 1024-point stride of a work-group (every NP with K1 = 8,
# every K1 with NP = 1028, C = 1 and B = 1 more than once)
MIX_CASES = [(3, 8, 3, 4), (1, 8, 40, 1020), (3, 8, 1, 1024), (3, 8, 3, 1028), (1, 8, 3, 2052),
             (3, 1, 40, 1028), (1, 2, 3, 1028), (3, 5, 1, 1028), (3, 2, 40, 2052)]

# (B, K1, C, reference_layout, B*K1*C > C*C: the backward's sums kernel has dpooled threads beyond the C*C weight threads)
COMPAT_CASES = [(1, 1, 36, True, False),       # K1 = 1: comp == 1, every gradient zero
                (2, 2, 17, True, False),       # one unrolled pass + one tail iteration
                (3, 6, 100, True, False),      # 6 unrolled passes + 4 tail iterations, two waves (the second partly) on
                (7, 7, 250, True, False),      # B and K1 not coprime; 15 passes + 10 tail iterations
                (7, 8, 4, True, True),         # tail loops only, B and K1 coprime, dpooled threads beyond C*C
                (7, 8, 1, False, True),        # one channel: every normalised vector is +-1
                (5, 3, 15, False, False),      # tail loops only, B*K1*C == C*C
                (2, 4, 63, True, False),       # one lane short of a wave
                (2, 4, 65, False, False),      # one lane into the second wave
                (6, 4, 256, True, False)]      # the widest the ABI admits, no tail
# (B, K1, C, reference_layout, (b0, k0)): descriptor row (b0, k0) is all zeros and bk = 0
COMPAT_DEGENERATE = [(3, 4, 40, True, (1, 2)), (3, 4, 40, False, (2, 3))]

RETRIEVAL_S = (2, 3)               # query shapes, candidate shapes
RETRIEVAL_NS = [(1, 1), (127, 129), (128, 128), (129, 127), (130, 257)]
RETRIEVAL_CS = [4, 36, 256, 260]
# every C with (127, 129), every (n1, n2) with C = 36
RETRIEVAL_CASES = [(127, 129, c) for c in RETRIEVAL_CS] + [(n1, n2, 36) for n1, n2 in RETRIEVAL_NS if (n1, n2) != (127, 129)]
RAGGED_CS = [4, 36, 260]
RAGGED_LENS = ([1, 127, 129], [128, 130])


def _randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------------
# the mix (combine.hip)
# ------------------------------------------------------------------------------------------------------
def mix_inputs(B, K1, C, NP, seed=0):
    """fp32 inputs of one mix case: xhat (B, K1, C, NP), comp (B, K1) a softmax, gamma, beta (C,), dfeats (B, C, NP)."""
    rng = np.random.default_rng(1000 * seed + 131 * B + 17 * K1 + 7 * C + NP)
    return {"xhat": _randn(rng, B, K1, C, NP), "comp": torch.softmax(_randn(rng, B, K1), dim=1), "gamma": _randn(rng, C),
            "beta": _randn(rng, C), "dfeats": _randn(rng, B, C, NP)}


def mix_fwd(xhat, comp, gamma, beta):
    """feats[b][c][n] = gamma[c] sum_k comp[b][k] xhat[b][k][c][n] + beta[c] sum_k comp[b][k], and the scale of its rounding
    error |gamma| sum_k |comp_k xhat_k| + |beta| sum_k |comp_k|.  xhat (B, K1, C, NP)."""
    xhat, comp, gamma, beta = (t.double() for t in (xhat, comp, gamma, beta))
    terms = comp[:, :, None, None] * xhat
    feats = gamma[None, :, None] * terms.sum(dim=1) + beta[None, :, None] * comp.sum(dim=1)[:, None, None]
    scale = gamma.abs()[None, :, None] * terms.abs().sum(dim=1) + beta.abs()[None, :, None] * comp.abs().sum(dim=1)[:, None, None]
    return feats, scale


def mix_bwd(dfeats, xhat, comp, gamma):
    """dxhat[b][k][c][n] = comp[b][k] gamma[c] dfeats[b][c][n]; rowdot[b][k][c] = sum_n dfeats xhat_k; rowsum[b][c] = sum_n dfeats;
    and the scales sum_n |dfeats xhat_k| (B, K1, C) and sum_n |dfeats| (B, C)."""
    dfeats, xhat, comp, gamma = (t.double() for t in (dfeats, xhat, comp, gamma))
    dxhat = comp[:, :, None, None] * gamma[None, None, :, None] * dfeats[:, None]
    prod = dfeats[:, None] * xhat
    return dxhat, prod.sum(dim=3), dfeats.sum(dim=2), prod.abs().sum(dim=3), dfeats.abs().sum(dim=2)


def mix_param_grads(rowdot, rowsum, comp, gamma, beta):
    """(dcomp (B, K1), dgamma (C,), dbeta (C,)) from the reductions, each as (value, sum of the absolute values of its terms):
    dcomp[b][k] = sum_c rowdot[b][k][c] gamma[c] + sum_c rowsum[b][c] beta[c];  dgamma[c] = sum_{b,k} comp[b][k] rowdot[b][k][c];
    dbeta[c] = sum_{b,k} comp[b][k] rowsum[b][c]."""
    rowdot, rowsum, comp, gamma, beta = (t.double() for t in (rowdot, rowsum, comp, gamma, beta))
    t_g, t_b = rowdot * gamma, rowsum * beta                                        # (B, K1, C), (B, C)
    dcomp = (t_g.sum(dim=2) + t_b.sum(dim=1, keepdim=True), t_g.abs().sum(dim=2) + t_b.abs().sum(dim=1, keepdim=True))
    t_c = comp[:, :, None] * rowdot
    dgamma = (t_c.sum(dim=(0, 1)), t_c.abs().sum(dim=(0, 1)))
    t_s = comp[:, :, None] * rowsum[:, None]
    dbeta = (t_s.sum(dim=(0, 1)), t_s.abs().sum(dim=(0, 1)))
    return dcomp, dgamma, dbeta


# ------------------------------------------------------------------------------------------------------
# the compatibility head (compat.hip)
# ------------------------------------------------------------------------------------------------------
def compat_inputs(B, K1, C, seed=0, zero_row=None):
    """fp32 inputs of one case: pooled (B, K1, C), wq, wk (C, C) of variance 1 / C, bq, bk (C,), dcomp (B, K1).  ``zero_row``
    (b0, k0): that descriptor is all zeros and bk = 0, so its projected key is exactly zero."""
    rng = np.random.default_rng(77000 + 1000 * seed + 131 * B + 17 * K1 + C)
    t = {"pooled": _randn(rng, B, K1, C), "wq": _randn(rng, C, C) / C ** 0.5, "bq": _randn(rng, C) * 0.1,
         "wk": _randn(rng, C, C) / C ** 0.5, "bk": _randn(rng, C) * 0.1, "dcomp": _randn(rng, B, K1)}
    if zero_row is not None:
        t["pooled"][zero_row[0], zero_row[1]] = 0.0
        t["bk"].zero_()
    return t


def compat_keys(pooled, reference_layout):
    """The key rows (B, K1, C) of the head: the reference's own bookkeeping (descriptors concatenated neighbour-major, then
    re-viewed), or every shape against its own neighbours."""
    B, K1, C = pooled.shape
    return pooled.transpose(0, 1).reshape(K1 * B, C).view(B, K1, C) if reference_layout else pooled


def _unkeys(dkeys, reference_layout):
    """Gradient of the key rows back onto the descriptors: the bookkeeping above read backwards."""
    B, K1, C = dkeys.shape
    return dkeys.reshape(K1 * B, C).view(K1, B, C).transpose(0, 1) if reference_layout else dkeys


def _unit(x):
    n = torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(EPS)
    return x / n, n


def compat_fwd(pooled, wq, bq, wk, bk, reference_layout):
    """comp (B, K1) = softmax_k <unit(Wq y_0 + bq), unit(Wk key_k + bk)>, unit(x) = x / max(|x|, 1e-12); every step written out
    (torch autograd can be taken of it from outside)."""
    pooled, wq, bq, wk, bk = (t.double() for t in (pooled, wq, bq, wk, bk))
    uq, _ = _unit(pooled[:, 0] @ wq.t() + bq)                                        # (B, C)
    uk, _ = _unit(compat_keys(pooled, reference_layout) @ wk.t() + bk)               # (B, K1, C)
    s = (uq[:, None, :] * uk).sum(dim=-1)
    e = torch.exp(s - s.amax(dim=1, keepdim=True))
    return e / e.sum(dim=1, keepdim=True)


def compat_scalar_tol(pooled, wq, bq, wk, bk, reference_layout, dcomp):
    """C = 1 only.  A normalised scalar is +-1 whatever its value, so every gradient of the head is exactly zero there, and what
    any floating-point backward returns is the rounding of the cancellation (du - u (u du)) / n.  In float64: u = 1 + d with
    |d| <= 2 * 2^-53 (the square root and the division), so |1 - u^2| <= 2^-51, and the two products and the difference add
    3 * 2^-53: at most 7 * 2^-53 |du| / n < 2^-50 |du| / n per row, with |du| <= |ds| <= 2 max |dcomp|.  A row reaches an output
    through one factor (a weight or a descriptor) and the outputs add at most B K1 rows, with roundings of their own and one to
    fp32 (another factor 2 covers both).  Returns 2^-48 B K1 max|dcomp| max(1, |pooled|, |w|) / min n: the absolute bound of
    every gradient of such a case (there is nothing to be relative to)."""
    pooled, wq, bq, wk, bk, dcomp = (t.double() for t in (pooled, wq, bq, wk, bk, dcomp))
    B, K1, C = pooled.shape
    assert C == 1
    _, nq = _unit(pooled[:, 0] @ wq.t() + bq)
    _, nk = _unit(compat_keys(pooled, reference_layout) @ wk.t() + bk)
    factor = max(1.0, pooled.abs().max().item(), wq.abs().max().item(), wk.abs().max().item())
    return 2.0 ** -48 * B * K1 * dcomp.abs().max().item() * factor / min(nq.min().item(), nk.min().item())


def compat(pooled, wq, bq, wk, bk, reference_layout, dcomp=None):
    """comp, and with ``dcomp`` the five gradients by hand: dict pooled, wq, bq, wk, bk."""
    comp = compat_fwd(pooled, wq, bq, wk, bk, reference_layout)
    if dcomp is None:
        return comp
    pooled, wq, bq, wk, bk, dcomp = (t.double() for t in (pooled, wq, bq, wk, bk, dcomp))
    y0, keys = pooled[:, 0], compat_keys(pooled, reference_layout)
    uq, nq = _unit(y0 @ wq.t() + bq)
    uk, nk = _unit(keys @ wk.t() + bk)
    ds = comp * (dcomp - (comp * dcomp).sum(dim=1, keepdim=True))                    # softmax
    duq = (ds[:, :, None] * uk).sum(dim=1)                                           # the dot products
    duk = ds[:, :, None] * uq[:, None, :]

    def unit_bwd(u, n, du):                                                          # below the clamp the division is by a constant
        return torch.where(n > EPS, (du - u * (u * du).sum(dim=-1, keepdim=True)) / n, du / EPS)

    drq, drk = unit_bwd(uq, nq, duq), unit_bwd(uk, nk, duk)                          # (B, C), (B, K1, C)
    dpooled = _unkeys(drk @ wk, reference_layout).clone()
    dpooled[:, 0] += drq @ wq
    return comp, {"pooled": dpooled, "wq": drq.t() @ y0, "bq": drq.sum(dim=0),
                  "wk": torch.einsum("bki,bkj->ij", drk, keys), "bk": drk.sum(dim=(0, 1))}


# ------------------------------------------------------------------------------------------------------
# the retrieval measure (retrieval.hip)
# ------------------------------------------------------------------------------------------------------
def normal_pair(n1, n2, C, seed=0, s=RETRIEVAL_S):
    rng = np.random.default_rng(5000 + 1000 * seed + 7 * n1 + 3 * n2 + C)
    return _randn(rng, s[0], n1, C), _randn(rng, s[1], n2, C)


def negative_pair(n1, n2, C, seed=0, s=RETRIEVAL_S):
    """queries |N(0, 1)|, candidates -|N(0, 1)|: every cosine, so every maximum and every score, is strictly negative."""
    f1, f2 = normal_pair(n1, n2, C, seed + 1, s)
    return f1.abs(), -f2.abs()


def ragged_shapes(C, negative=False):
    """Query and candidate shapes (lists of (n, C) fp32 rows) of the ragged cases, lengths RAGGED_LENS."""
    make = negative_pair if negative else normal_pair
    qs = [make(n, 1, C, seed=10 + i, s=(1, 1))[0][0] for i, n in enumerate(RAGGED_LENS[0])]
    ks = [make(1, n, C, seed=20 + j, s=(1, 1))[1][0] for j, n in enumerate(RAGGED_LENS[1])]
    return qs, ks


def retrieval(f1, f2):
    """r[i][j] = mean_n max_m cos(f1[i][n], f2[j][m]), rows normalised as x / max(|x|, 1e-12).  f1 (S1, N1, C), f2 (S2, N2, C)."""
    u1, _ = _unit(f1.double())
    u2, _ = _unit(f2.double())
    return torch.stack([torch.stack([(a @ b.t()).amax(dim=1).mean() for b in u2]) for a in u1])


def retrieval_bound(C, n1):
    """Worst-case |error| of one score in fp32: a dot product of C terms between unit-scale vectors, two norms, two reciprocals
    and two scalings, the 256-way strided sum and the tree of the mean (the maximum is 1-Lipschitz)."""
    return (C + n1 / 256 + 32) * U
