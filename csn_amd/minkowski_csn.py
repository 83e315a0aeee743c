"""The cross-shape head of MinkowskiNet's ``HRNetSimCSN`` and its shape graph on ragged shape batches, on the MI355X kernels.

Reference (marios2019/CSN):
  * ``HRNetSimCSN`` head           MinkowskiNet/models/hrnet.py:341-357 (parameters), 359-423 (forward), 456-470 (get_SSA)
  * ``cosine_similarity``          MinkowskiNet/models/hrnet.py:472-490
  * ``construct_shape_graph``      MinkowskiNet/lib/csn_utils.py:11-111 (random branch :31-43, similarity branch :44-97)

The reference runs the head as a Python loop over the query shapes: 2K+1 separate ``MultiHeadAttention`` calls per shape, the
pooling, compatibility and mix in eager torch on each shape's rows, and a shape graph built from an O(S^2) loop of
``cosine_similarity`` calls that each build the full n x m cosine matrix.  Here one forward is:

  1. ONE varlen attention call (``_CrossMHA`` with q_lens / k_lens) for all B (2K+1) evaluations, ordered
        S_b = MHA(q_b, q_b, q_b)                     e = b
        T_{i,b} = MHA(k_{i,b}, k_{i,b}, k_{i,b})     e = B + i B + b
        X_{i,b} = MHA(q_b, k_{i,b}, k_{i,b})         e = B + K B + i B + b
     S_b is evaluated once and serves the pooling and the mix (one dropout mask in train mode).  The layer leaves the
     channel-major, pre-affine LayerNorm output xhat; the affine is never materialised per evaluation.
  2. ``csn_ragged_pool_f32``: the pooled descriptors gamma * mean_n xhat + beta of S and T, over each evaluation's EXACT
     point count (the varlen attention ran round-up-4 queries; the points beyond the count hold real values and are skipped).
  3. the (B, K+1, C) compatibility math (linear_q, linear_k, normalize, ``ScaledDotProduct``, softmax): torch ops on
     2 (K+1) C^2 FLOP per shape, differentiated by autograd inside the head's backward.
  4. ``csn_ragged_mix_fwd_f32``: sum_j comp_j (gamma xhat + beta) written point-major straight into the csa half of the
     (N, 2 d_model) input of ``output``; the query half is a copy of q, so ``cat([q, csa])`` costs nothing more.
  5. ``output``: one (N, 2 d_model) x (2 d_model, out_channels) GEMM through ``F.linear``.  The project's GEMM entry points take
     channel-major maps; this product is point-major on both sides, so it goes to the platform BLAS rather than through two
     transposes.
Backward: ``csn_ragged_mix_bwd_f32`` (the mixed maps' gradients and the fp64 per-(shape, slot, channel) dot products from
which d comp, d gamma, d beta follow), the compatibility math's autograd, then ``csn_ragged_pool_bwd_f32`` (the pooled
descriptors' share, added to S and written for T), then the attention backward.

The HRNet backbone is ``minkowski_hrnet.py`` (``HRNetSimCSN2S`` / ``3S`` feed this head): inputs are the backbone features after ``fc_layer``, packed
point-major rows sorted by shape plus their offsets (``offsets_from_batch_index`` derives them from an ME batch column) — or,
for a head built with ``backbone_channels``, the concatenated backbone map itself: the head then owns ``fc_layer``
(``BackboneFC``: hrnet.py:332-339, the kernel-size-1 convolution + BatchNorm + ReLU on ``csn_rows_fc_fwd_f32`` / ``_bwd_f32``) and
applies it to the query batch and to every key batch, one BatchNorm batch each, as hrnet.py:439 and :451 do.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import functional as CF
from . import tuning
from .minkowski_attention import MultiHeadAttention, ScaledDotProduct, _CrossMHA, _up

LN_WIDTHS = (32, 64, 96, 128, 256)          # d_model instances of the LayerNorm epilogues (DESIGN §1 "Not supported")

Ragged = Tuple[torch.Tensor, Sequence[int]]   # (rows (N, C), offsets (B + 1))


# ------------------------------------------------------------------------------------------------------
# offsets and host-side helpers
# ------------------------------------------------------------------------------------------------------
def offsets_from_batch_index(batch_index, n_shapes: Optional[int] = None) -> torch.Tensor:
    """Offsets (B + 1, int64, CPU) of packed rows from an ME-style batch-index column (``coords[:, 0]``).  The rows must be
    sorted by shape: the reference's final ``torch.cat`` (hrnet.py:413-421) silently assumes it, so an unsorted column
    raises here.  Every shape needs at least one row."""
    b = torch.as_tensor(batch_index).reshape(-1).to("cpu", torch.int64)
    if b.numel() == 0:
        raise ValueError("empty batch-index column")
    if (b[1:] < b[:-1]).any():
        raise ValueError("batch-index column is not non-decreasing: the rows are not sorted by shape")
    if b[0] < 0:
        raise ValueError("negative batch index")
    B = int(b[-1]) + 1 if n_shapes is None else int(n_shapes)
    counts = torch.bincount(b, minlength=B)
    if counts.numel() != B or (counts == 0).any():
        raise ValueError("every shape of the batch needs at least one row")
    return torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])


def _host_offsets(offsets, n_rows: int) -> List[int]:
    off = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    if len(off) < 2 or off[0] != 0 or off[-1] != n_rows or any(b <= a for a, b in zip(off, off[1:])):
        raise ValueError("offsets must start at 0, increase strictly (every shape >= 1 row) and end at the row count")
    return off


def _int32_pair(values: Sequence[int], dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same int32 numbers on the host (validated by the C ABI, sizes the grid) and on the device (read by the kernels)."""
    h = torch.tensor(list(values), dtype=torch.int32)
    return h, h.to(dev, non_blocking=False)


def topk_neighbors(similarity, K: int, is_same: bool) -> List[Tuple[int, List[int]]]:
    """The neighbour rule of csn_utils.py:91-96 on a (S_q, S_k) similarity matrix: ``topk(K)``; when the keys are the queries
    and the query is among them, ``topk(K + 1)`` with the query dropped.  Host-only (CPU tensors, torch's own topk)."""
    sim = torch.as_tensor(similarity).detach().to("cpu")
    out = []
    for q_idx in range(sim.shape[0]):
        _, indices = torch.topk(sim[q_idx], K)
        if is_same and q_idx in indices:
            _, indices = torch.topk(sim[q_idx], K + 1)
            indices = indices[q_idx != indices]
        out.append((q_idx, indices.tolist()))
    return out


def random_neighbors(n_query: int, n_key: int, K: int, is_same: bool, rng: np.random.Generator) -> List[Tuple[int, List[int]]]:
    """csn_utils.py:31-43 with an explicit numpy Generator: K distinct keys per query, redrawn while the query itself is among
    them (keys are the queries)."""
    if K < 1 or K > n_key - (1 if is_same else 0):
        raise ValueError(f"cannot draw {K} distinct neighbours from {n_key} shapes")
    out = []
    for idx in range(n_query):
        indices = rng.choice(n_key, K, replace=False)
        while is_same and idx in indices:
            indices = rng.choice(n_key, K, replace=False)
        out.append((idx, [int(i) for i in indices]))
    return out


# ------------------------------------------------------------------------------------------------------
# ragged retrieval
# ------------------------------------------------------------------------------------------------------
def retrieval_measure_ragged(f1: torch.Tensor, offsets1, f2: torch.Tensor, offsets2, pair_budget: int = 2 ** 26) -> torch.Tensor:
    """r[i][j] = mean_{n < n_i} max_{m < m_j} cos(f1_i[n], f2_j[m]) for packed point-major rows with offsets (hrnet.py:472-490
    for every pair; rows normalised with the 1e-12 clamp of F.normalize).  (S1, S2) fp32.  The scratch is N1 + N2 + pairs x
    query tiles floats; query shapes are scored in row chunks of at most ``pair_budget`` pair tiles."""
    CF._need_cuda(f1, f2)
    f1, f2 = f1.contiguous(), f2.contiguous()
    o1, o2 = _host_offsets(offsets1, f1.shape[0]), _host_offsets(offsets2, f2.shape[0])
    S1, S2, C = len(o1) - 1, len(o2) - 1, f1.shape[1]
    if f2.shape[1] != C:
        raise ValueError("both feature sets need the same channel count")
    dev = f1.device
    out = torch.empty((S1, S2), device=dev, dtype=torch.float32)
    h2, d2 = _int32_pair(o2, dev)
    lens1 = [b - a for a, b in zip(o1, o1[1:])]
    i = 0
    while i < S1:
        # rows [i, j): tiles of the longest of them times S2 within the budget (at least one row)
        j, mx = i + 1, lens1[i]
        while j < S1 and (j + 1 - i) * S2 * ((max(mx, lens1[j]) + 127) // 128) <= pair_budget:
            mx = max(mx, lens1[j])
            j += 1
        sub = [o - o1[i] for o in o1[i:j + 1]]
        h1, d1 = _int32_pair(sub, dev)
        ws_n = sub[-1] + o2[-1] + (j - i) * S2 * ((mx + 127) // 128)
        ws = torch.empty((ws_n,), device=dev, dtype=torch.float32)
        _lib.check(_lib.lib().csn_ragged_retrieval_f32(CF._ptr(f1[o1[i]:o1[j]]), h1.data_ptr(), CF._ptr(d1), j - i, CF._ptr(f2),
                                                       h2.data_ptr(), CF._ptr(d2), S2, C, CF._ptr(out[i:j]), CF._ptr(ws), ws_n,
                                                       CF._stream()), "csn_ragged_retrieval_f32")
        i = j
    return out


# ------------------------------------------------------------------------------------------------------
# exact top-K retrieval behind an fp16 screen
# ------------------------------------------------------------------------------------------------------
SCREEN_MAX_CHANNELS = 288                    # round-up-32(C) the screen kernel's LDS images hold (include/csn_hip.h, section 11b)
# An element beyond this magnitude (or a non-finite one) can overflow the fp32 measure's own sums: screen_eps bounds the distance
# to the fp32 measure only where that measure stays in range.  Such a shape is never screened out, its own row is scored in full,
# and its screen scores never enter another row's threshold (screen_shortlist).
_SCREEN_SAFE_MAX = 2.0 ** 55


def screen_eps(C: int) -> float:
    """The DERIVED bound of the fp16 screen: |retrieval_screen_ragged - retrieval_measure_ragged| <= screen_eps(C) for every pair
    (``csn_retrieval_screen_eps``; derivation in DESIGN.md "fp16 screen of the shape graph")."""
    return float(_lib.lib().csn_retrieval_screen_eps(int(C)))


def _ragged_args(f1, offsets1, f2, offsets2):
    CF._need_cuda(f1, f2)
    f1, f2 = f1.contiguous(), f2.contiguous()
    o1, o2 = _host_offsets(offsets1, f1.shape[0]), _host_offsets(offsets2, f2.shape[0])
    if f2.shape[1] != f1.shape[1]:
        raise ValueError("both feature sets need the same channel count")
    return f1, o1, f2, o2


def _row_chunks(lens1: Sequence[int], S2: int, pair_budget: int):
    """Query rows [i, j) whose pair tiles (S2 x tiles of the longest of them) stay within the budget, at least one row each."""
    i, S1 = 0, len(lens1)
    while i < S1:
        j, mx = i + 1, lens1[i]
        while j < S1 and (j + 1 - i) * S2 * ((max(mx, lens1[j]) + 127) // 128) <= pair_budget:
            mx = max(mx, lens1[j])
            j += 1
        yield i, j, mx
        i = j


def retrieval_screen_ragged(f1: torch.Tensor, offsets1, f2: torch.Tensor, offsets2, pair_budget: int = 2 ** 26) -> torch.Tensor:
    """The fp16 SCREEN of ``retrieval_measure_ragged``: the same (S1, S2) fp32 matrix within ``screen_eps(C)`` of it, from unit
    rows rounded once to fp16 on the 16-bit matrix cores (``csn_ragged_retrieval_screen_f16``).  It ranks nothing: it tells
    ``topk_retrieval_ragged`` which pairs need no exact score."""
    f1, o1, f2, o2 = _ragged_args(f1, offsets1, f2, offsets2)
    S1, S2, C = len(o1) - 1, len(o2) - 1, f1.shape[1]
    if (C + 31) // 32 * 32 > SCREEN_MAX_CHANNELS:
        raise _lib.CsnError(f"the retrieval screen holds up to {SCREEN_MAX_CHANNELS} channels (got {C}); score exactly instead")
    dev, L = f1.device, _lib.lib()
    out = torch.empty((S1, S2), device=dev, dtype=torch.float32)
    h2, d2 = _int32_pair(o2, dev)
    lens1 = [b - a for a, b in zip(o1, o1[1:])]
    for i, j, mx in _row_chunks(lens1, S2, pair_budget):
        sub = [o - o1[i] for o in o1[i:j + 1]]
        h1, d1 = _int32_pair(sub, dev)
        ws_n = int(L.csn_retrieval_screen_workspace_floats(sub[-1], o2[-1], j - i, S2, mx, C))
        ws = torch.empty((ws_n,), device=dev, dtype=torch.float32)
        _lib.check(L.csn_ragged_retrieval_screen_f16(CF._ptr(f1[o1[i]:o1[j]]), h1.data_ptr(), CF._ptr(d1), j - i, CF._ptr(f2),
                                                     h2.data_ptr(), CF._ptr(d2), S2, C, CF._ptr(out[i:j]), CF._ptr(ws), ws_n,
                                                     CF._stream()), "csn_ragged_retrieval_screen_f16")
    return out


def retrieval_pairs_ragged(f1: torch.Tensor, offsets1, f2: torch.Tensor, offsets2, pairs: torch.Tensor,
                           pair_budget: int = 2 ** 26) -> torch.Tensor:
    """The exact fp32 measure of the listed pairs only: ``pairs`` (P, 2) integer (i, j) on the device, any order, repeats allowed
    -> (P,) fp32 with the bits ``retrieval_measure_ragged(...)[i, j]`` has (``csn_ragged_retrieval_pairs_f32``: the same
    work-groups, the pair looked up)."""
    f1, o1, f2, o2 = _ragged_args(f1, offsets1, f2, offsets2)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64):
        raise ValueError("pairs must be a (P, 2) int32 / int64 tensor of (query shape, key shape) indices")
    if not pairs.is_cuda:
        raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    S1, S2, C = len(o1) - 1, len(o2) - 1, f1.shape[1]
    dev, L = f1.device, _lib.lib()
    pairs = pairs.to(torch.int32).contiguous()
    P = pairs.shape[0]
    out = torch.empty((P,), device=dev, dtype=torch.float32)
    if P == 0:
        return out
    h1, d1 = _int32_pair(o1, dev)
    h2, d2 = _int32_pair(o2, dev)
    tiles = (max(b - a for a, b in zip(o1, o1[1:])) + 127) // 128
    step = max(1, pair_budget // tiles)
    for p0 in range(0, P, step):
        n = min(step, P - p0)
        ws_n = o1[-1] + o2[-1] + n * tiles
        ws = torch.empty((ws_n,), device=dev, dtype=torch.float32)
        _lib.check(L.csn_ragged_retrieval_pairs_f32(CF._ptr(f1), h1.data_ptr(), CF._ptr(d1), S1, CF._ptr(f2), h2.data_ptr(), CF._ptr(d2),
                                                    S2, C, CF._ptr(pairs[p0:p0 + n]), n, CF._ptr(out[p0:p0 + n]), CF._ptr(ws), ws_n,
                                                    CF._stream()), "csn_ragged_retrieval_pairs_f32")
    return out


def _unscreenable(f: torch.Tensor, off: Sequence[int]) -> torch.Tensor:
    """(S,) bool on the device: shapes holding a non-finite element or one beyond ``_SCREEN_SAFE_MAX``."""
    bad = (~(f.abs().amax(dim=1) <= _SCREEN_SAFE_MAX)).to(torch.int64).cumsum(0)
    bad = torch.cat([bad.new_zeros(1), bad])
    o = torch.tensor(list(off), dtype=torch.int64, device=f.device)
    return (bad[o[1:]] - bad[o[:-1]]) > 0


def screen_shortlist(screen: torch.Tensor, k_top: int, eps: float, wild: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The selection rule on a (rows, S2) block of screen scores: keep a candidate iff its score is >= t - 2 eps, t = the k_top-th
    largest score of its row.  Bool mask, same device.  With |screen - exact| <= eps a dropped candidate is strictly below k_top
    others in exact arithmetic: it is in no top-k_top of the exact scores.  ``wild`` (S2,) bool marks the candidates the bound does
    NOT cover: they are always kept and they take no part in t — the k_top scores that justify a drop must themselves be within
    eps of their exact scores (a wild candidate's screen score can lie far above its exact one and would lift t).  A row with
    fewer than k_top covered candidates, or with a non-finite score among them, keeps every candidate.
    (Compared in fp64, where t - 2 eps is exact: an fp32 difference could round the threshold up.)"""
    s = screen.double()
    if wild is None:
        wild = torch.zeros(screen.shape[1], dtype=torch.bool, device=screen.device)
    s = s.masked_fill(wild[None, :], float("-inf"))
    t = torch.topk(s, k_top, dim=1).values[:, -1:]              # -inf where fewer than k_top covered candidates: keeps the row
    keep = (s >= t - 2.0 * float(eps)) | wild[None, :]
    return keep | (~torch.isfinite(screen) & ~wild[None, :]).any(dim=1, keepdim=True)


def topk_retrieval_ragged(f1: torch.Tensor, offsets1, f2: torch.Tensor, offsets2, K: int, is_same: bool,
                          pair_budget: int = 2 ** 26) -> Tuple[List[Tuple[int, List[int]]], dict]:
    """``topk_neighbors(retrieval_measure_ragged(f1, offsets1, f2, offsets2), K, is_same)`` — the same list of integers — without
    the exact score of every pair.  Per chunk of query rows: the fp16 screen of the chunk; the shortlist of ``screen_shortlist``
    with K' = K + 1 when ``is_same`` (the query itself may have to be dropped, csn_utils.py:91-96), else K; the exact fp32 score
    of the shortlisted pairs (``retrieval_pairs_ragged``) scattered into a matrix of -inf; ``topk_neighbors`` on the result.
    Selection stays on the device; one host read per chunk (the pair count).  A shape with a non-finite or huge (> 2^55) element
    is outside the bound: as a query its row is scored in full, as a key it is always scored and takes no part in the row's
    threshold.  A row with a non-finite screen score is scored in full; fewer than K' keys take the all-pairs path and raise
    what it raises.  ``stats``: pairs screened, pairs re-scored exactly, the largest shortlist of a row."""
    f1, o1, f2, o2 = _ragged_args(f1, offsets1, f2, offsets2)
    S1, S2, C = len(o1) - 1, len(o2) - 1, f1.shape[1]
    k_top = K + 1 if is_same else K
    if S2 < k_top or K < 1:
        sim = retrieval_measure_ragged(f1, o1, f2, o2, pair_budget)
        return topk_neighbors(sim.cpu(), K, is_same), {"pairs_screened": 0, "pairs_rescored": S1 * S2, "max_shortlist": S2}
    eps = screen_eps(C)
    wild_q, wild_k = _unscreenable(f1, o1), _unscreenable(f2, o2)
    lens1 = [b - a for a, b in zip(o1, o1[1:])]
    blocks, rescored, longest = [], 0, torch.zeros((), dtype=torch.int64, device=f1.device)
    for i, j, _ in _row_chunks(lens1, S2, pair_budget):
        sub = [o - o1[i] for o in o1[i:j + 1]]
        rows = f1[o1[i]:o1[j]]
        screen = retrieval_screen_ragged(rows, sub, f2, o2, pair_budget)
        keep = screen_shortlist(screen, k_top, eps, wild_k) | wild_q[i:j, None]
        pairs = keep.nonzero()                                  # the chunk's one host read: the pair count
        longest = torch.maximum(longest, keep.sum(dim=1).max())
        rescored += pairs.shape[0]
        full = torch.full((j - i, S2), float("-inf"), device=f1.device, dtype=torch.float32)
        full[pairs[:, 0], pairs[:, 1]] = retrieval_pairs_ragged(rows, sub, f2, o2, pairs, pair_budget)
        blocks.append(full.cpu())
    stats = {"pairs_screened": S1 * S2, "pairs_rescored": rescored, "max_shortlist": int(longest)}
    return topk_neighbors(torch.cat(blocks), K, is_same), stats


SCREEN_MAX_POINTS = 61000                    # points per shape the fixed-length measure's fp32 mean stays inside screen_eps for


def knn_graph_screened(f1: torch.Tensor, f2: torch.Tensor, K: int, pair_budget: int = 2 ** 26) -> Tuple[torch.Tensor, dict]:
    """``csn_amd.functional.retrieval_measure(f1, f2).topk(K + 1, -1).indices`` for fixed-length point-major features (S1, N1, C),
    (S2, N2, C) — MID-FC's get_knn_graph — behind the same screen: the features are a ragged set with uniform offsets, K' = K + 1,
    and the shortlisted candidates of a query are scored by the fixed-length fp32 kernel itself (a pair's bits there depend on
    the pair alone), so the (S1, K + 1) int64 tensor is the one the all-pairs path returns.  One host read per call."""
    CF._need_cuda(f1, f2)
    S1, N1, C = f1.shape
    S2, N2, _ = f2.shape
    if S2 < K + 1:
        return CF.retrieval_measure(f1, f2).topk(K + 1, -1)[1], {"pairs_screened": 0, "pairs_rescored": S1 * S2, "max_shortlist": S2}
    if N1 > SCREEN_MAX_POINTS:
        raise _lib.CsnError(f"the retrieval screen's bound covers up to {SCREEN_MAX_POINTS} points per query shape (got {N1})")
    f1, f2 = f1.contiguous(), f2.contiguous()
    r1, r2 = f1.reshape(S1 * N1, C), f2.reshape(S2 * N2, C)
    o1, o2 = [i * N1 for i in range(S1 + 1)], [i * N2 for i in range(S2 + 1)]
    screen = retrieval_screen_ragged(r1, o1, r2, o2, pair_budget)
    keep = screen_shortlist(screen, K + 1, screen_eps(C), _unscreenable(r2, o2)) | _unscreenable(r1, o1)[:, None]
    full = torch.full((S1, S2), float("-inf"), device=f1.device, dtype=torch.float32)
    pairs = keep.nonzero()                                      # the call's one host read (row-major: a query's candidates adjoin)
    counts = torch.bincount(pairs[:, 0], minlength=S1).tolist()
    at = 0
    for q, n in enumerate(counts):
        cols = pairs[at:at + n, 1]
        full[q, cols] = CF.retrieval_measure(f1[q:q + 1], f2[cols])[0]
        at += n
    stats = {"pairs_screened": S1 * S2, "pairs_rescored": pairs.shape[0], "max_shortlist": max(counts)}
    return full.topk(K + 1, -1)[1], stats


# ------------------------------------------------------------------------------------------------------
# the head's pool / compatibility / mix as one autograd node
# ------------------------------------------------------------------------------------------------------
class _RaggedHead(torch.autograd.Function):
    """(xhat (E, C, ld) of the evaluation order above, q_rows (N, C)) -> out (N, 2C) = [q | csa], or (N, C) = the SSA rows
    (``ssa_only``).  K = 0 / ssa_only: csa = S (k1 = 1, comp = 1, no pooling)."""

    @staticmethod
    def forward(ctx, xhat, gamma, beta, wq, wk, q_rows, plan):
        L = _lib.lib()
        E, C, ld = xhat.shape
        B, K, N = plan["B"], plan["K"], q_rows.shape[0]
        dev = xhat.device
        mixing = K > 0 and not plan["ssa_only"]
        k1 = K + 1 if mixing else 1
        gamma_c, beta_c = gamma.detach().contiguous(), beta.detach().contiguous()
        if plan["ssa_only"]:
            out = torch.empty((N, C), device=dev, dtype=torch.float32)
            csa = out
        else:
            out = torch.empty((N, 2 * C), device=dev, dtype=torch.float32)
            out[:, :C] = q_rows
            csa = out[:, C:]
        mean = graph = None
        if mixing:
            n_pool = B * (K + 1)
            pooled = torch.empty((n_pool, C), device=dev, dtype=torch.float32)
            mean = torch.empty((n_pool, C), device=dev, dtype=torch.float32)
            ch, cd = plan["counts"]
            _lib.check(L.csn_ragged_pool_f32(CF._ptr(xhat), C * ld, ld, ch.data_ptr(), CF._ptr(cd), n_pool, C, CF._ptr(gamma_c),
                                             CF._ptr(beta_c), CF._ptr(pooled), CF._ptr(mean), CF._stream()), "csn_ragged_pool_f32")
            with torch.enable_grad():
                p = pooled.view(K + 1, B, C).transpose(0, 1).detach().requires_grad_(True)       # (B, K+1, C), slot 0 = S_b
                wq_l, wk_l = wq.detach().requires_grad_(True), wk.detach().requires_grad_(True)
                u = F.normalize(F.linear(p[:, 0], wq_l), dim=-1)                                 # hrnet.py:382-383
                w = F.normalize(F.linear(p, wk_l), dim=-1)                                       # :390-391
                sim = plan["sim"](u.unsqueeze(1), w).squeeze(1)                                  # :393  (B, K+1)
                comp_g = F.softmax(sim, dim=-1)                                                  # :397
            comp = comp_g.detach().contiguous()
            graph = (comp_g, p, wq_l, wk_l)
        else:
            comp = torch.ones((B, 1), device=dev, dtype=torch.float32)
        oh, od = plan["offsets"]
        _lib.check(L.csn_ragged_mix_fwd_f32(CF._ptr(xhat), C * ld, ld, E, plan["cross_first"], oh.data_ptr(), CF._ptr(od), B, k1, C,
                                            CF._ptr(comp), CF._ptr(gamma_c), CF._ptr(beta_c), CF._ptr(csa), out.shape[1],
                                            CF._stream()), "csn_ragged_mix_fwd_f32")
        ctx.save_for_backward(xhat, gamma_c, beta_c, comp, mean)
        ctx.graph, ctx.plan, ctx.k1, ctx.mixing = graph, plan, k1, mixing
        return out

    @staticmethod
    def backward(ctx, dout):
        xhat, gamma, beta, comp, mean = ctx.saved_tensors
        plan, k1, mixing = ctx.plan, ctx.k1, ctx.mixing
        L = _lib.lib()
        E, C, ld = xhat.shape
        B, K = plan["B"], plan["K"]
        dev = xhat.device
        dout = dout.contiguous()
        dq = None if plan["ssa_only"] else dout[:, :C]
        dcsa = dout if plan["ssa_only"] else dout[:, C:]
        dxhat = torch.empty_like(xhat)
        rowdot = torch.empty((B, k1, C), device=dev, dtype=torch.float64)
        rowsum = torch.empty((B, C), device=dev, dtype=torch.float64)
        ws_n = B * (k1 + 1) * ((ld + 63) // 64) * C
        ws = torch.empty((ws_n,), device=dev, dtype=torch.float64)
        oh, od = plan["offsets"]
        _lib.check(L.csn_ragged_mix_bwd_f32(CF._ptr(dcsa), dout.shape[1], CF._ptr(xhat), C * ld, ld, E, plan["cross_first"],
                                            oh.data_ptr(), CF._ptr(od), B, k1, C, CF._ptr(comp), CF._ptr(gamma), CF._ptr(dxhat),
                                            CF._ptr(rowdot), CF._ptr(rowsum), CF._ptr(ws), ws_n, CF._stream()),
                   "csn_ragged_mix_bwd_f32")
        g64, b64, c64 = gamma.double(), beta.double(), comp.double()
        dgamma = torch.einsum("bj,bjc->c", c64, rowdot)
        dbeta = (c64.sum(dim=1, keepdim=True) * rowsum).sum(dim=0)
        dwq = dwk = None
        if mixing:
            dcomp = (rowdot * g64).sum(dim=2) + (rowsum * b64).sum(dim=1, keepdim=True)           # (B, K+1)
            comp_g, p, wq_l, wk_l = ctx.graph
            dp, dwq, dwk = torch.autograd.grad(comp_g, (p, wq_l, wk_l), dcomp.float())
            dpooled = dp.transpose(0, 1).reshape(B * (K + 1), C).contiguous()                    # evaluation order
            dgamma = dgamma + (dpooled.double() * mean.double()).sum(dim=0)
            dbeta = dbeta + dpooled.double().sum(dim=0)
            ch, cd = plan["counts"]
            # S_b: add to the mix's gradient; T_{i,b}: not mixed, written here (zero past each count)
            for first, n, acc in ((0, B, 1), (B, B * K, 0)):
                _lib.check(L.csn_ragged_pool_bwd_f32(CF._ptr(dpooled[first:]), CF._ptr(gamma), ch[first:].data_ptr(),
                                                     CF._ptr(cd[first:]), n, C, CF._ptr(dxhat[first:]), C * ld, ld, acc,
                                                     CF._stream()), "csn_ragged_pool_bwd_f32")
            ctx.graph = None
        return dxhat, dgamma.float(), dbeta.float(), dwq, dwk, dq, None


# ------------------------------------------------------------------------------------------------------
# fc_layer: kernel-size-1 convolution + BatchNorm + ReLU on point-major rows
# ------------------------------------------------------------------------------------------------------
class _RowsFC(torch.autograd.Function):
    """y = relu(batch_norm(x w^T + b)) through ``csn_rows_fc_fwd_f32`` / ``csn_rows_fc_bwd_f32``; one call is one BatchNorm
    batch.  Training updates ``running_mean`` / ``running_var`` in place."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, eps, momentum, training):
        CF._need_cuda(x, w, b, gamma, beta, running_mean, running_var)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        ctx.rows16 = tuning.current().rows_single_product
        x = x.contiguous()
        w_c, b_c, g_c, be_c = (t.detach().contiguous() for t in (w, b, gamma, beta))
        N, c_in = x.shape
        C = w_c.shape[0]
        dev = x.device
        y = torch.empty((N, C), device=dev, dtype=torch.float32)
        z = mean = invstd = ws = None
        ws_n = 0
        if training:
            z = torch.empty((N, C), device=dev, dtype=torch.float32)
            mean = torch.empty((C,), device=dev, dtype=torch.float32)
            invstd = torch.empty((C,), device=dev, dtype=torch.float32)
            ws_n = int(L.csn_rows_fc_workspace_bytes(N, c_in, C, 1, 0))
            ws = torch.empty((max(ws_n, 16),), device=dev, dtype=torch.uint8)
        with CF.rows16(ctx.rows16):                                        # training and eval (the folded epilogue) alike
            _lib.check(L.csn_rows_fc_fwd_f32(CF._ptr(x), c_in, N, c_in, C, CF._ptr(w_c), CF._ptr(b_c), CF._ptr(g_c), CF._ptr(be_c),
                                             CF._ptr(running_mean), CF._ptr(running_var), float(eps), float(momentum), int(training),
                                             CF._ptr(y), C, CF._ptr(z), C, CF._ptr(mean), CF._ptr(invstd), CF._ptr(ws), ws_n,
                                             CF._stream()), "csn_rows_fc_fwd_f32")
        if training:
            ctx.save_for_backward(x, w_c, b_c, g_c, y, z, mean, invstd)
        else:
            ctx.save_for_backward(x, w_c, b_c, g_c, y, None, running_mean.clone(), running_var.clone())
        ctx.training, ctx.eps = bool(training), float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        with CF.math_mode(CF.backward_mode(ctx.mode)), CF.rows16(ctx.rows16):
            x, w, b, gamma, y, z, s_mean, s_scale = ctx.saved_tensors
            L = _lib.lib()
            N, c_in = x.shape
            C = w.shape[0]
            dev = x.device
            dy = dy.contiguous()
            need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
            dx = torch.empty_like(x) if need_x else None
            dw = torch.empty_like(w) if need_w else None
            db = torch.empty((C,), device=dev, dtype=torch.float32) if need_b else None
            dgamma = torch.empty((C,), device=dev, dtype=torch.float32)
            dbeta = torch.empty((C,), device=dev, dtype=torch.float32)
            ws_n = int(L.csn_rows_fc_workspace_bytes(N, c_in, C, int(ctx.training), 1))
            ws = torch.empty((ws_n,), device=dev, dtype=torch.uint8)
            _lib.check(L.csn_rows_fc_bwd_f32(CF._ptr(dy), C, CF._ptr(y), C, CF._ptr(z), C, CF._ptr(x), c_in, N, c_in, C, CF._ptr(w),
                                             CF._ptr(b), CF._ptr(gamma), CF._ptr(s_mean), CF._ptr(s_scale), ctx.eps,
                                             int(ctx.training), CF._ptr(dx), c_in, CF._ptr(dw), CF._ptr(db), CF._ptr(dgamma),
                                             CF._ptr(dbeta), CF._ptr(ws), ws_n, CF._stream()), "csn_rows_fc_bwd_f32")
            return dx, dw, db, dgamma, dbeta, None, None, None, None, None


class BackboneFC(nn.Sequential):
    """``fc_layer`` of hrnet.py:332-339 on dense rows: ``nn.Linear(in_channels, d_model)`` (the kernel-size-1
    MinkowskiConvolution with bias), ``nn.BatchNorm1d(d_model, momentum=bn_momentum)`` (lib/config.py:63 gives 0.02) and
    ``nn.ReLU`` — as holders of parameters and buffers only: ``forward`` runs the three as one autograd node on the HIP kernels.
    BatchNorm weight 1 and bias 0 at construction (hrnet.py:165-169).  One call is one BatchNorm batch over its (N, in_channels)
    rows; a training call with one row raises ``ValueError`` as torch does."""

    def __init__(self, in_channels: int, d_model: int, bn_momentum: float = 0.02, eps: float = 1e-5):
        if d_model not in LN_WIDTHS:
            raise ValueError(f"d_model {d_model} is not supported: the kernels are built for d_model in {LN_WIDTHS}")
        if in_channels % 32 or not 32 <= in_channels <= 1024:
            raise ValueError(f"in_channels {in_channels} is not supported: a multiple of 32 in [32, 1024]")
        super().__init__(nn.Linear(in_channels, d_model, bias=True), nn.BatchNorm1d(d_model, eps=eps, momentum=bn_momentum), nn.ReLU())
        nn.init.constant_(self[1].weight, 1.0)
        nn.init.constant_(self[1].bias, 0.0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fc, bn = self[0], self[1]
        if not x.is_cuda:
            raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        if x.dim() != 2 or x.shape[1] != fc.in_features:
            raise ValueError(f"rows must be (N, {fc.in_features})")
        if self.training and x.shape[0] == 1:
            raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
        if self.training:
            bn.num_batches_tracked += 1
        return _RowsFC.apply(x.float(), fc.weight, fc.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                             bn.momentum, self.training)


# ------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------
class SimCSNHead(nn.Module):
    """The cross-shape head of ``HRNetSimCSN`` (hrnet.py:341-423) on dense backbone features.  Submodules and parameters as
    at hrnet.py:341-357: ``MHA`` (``MultiHeadAttention(n_head, d_model, d_model // n_head, d_model // n_head)``), ``output``
    (``nn.Linear(2 d_model, out_channels)``: the kernel-size-1 MinkowskiConvolution of :346-351 on dense rows) and, when
    ``k_neighbors > 0``, ``linear_q`` / ``linear_k`` (no bias) and ``sim`` (``ScaledDotProduct(d_model ** 0.5)``).

    ``forward(q, q_offsets, keys=None, return_ssa=False)``: q (N, d_model) point-major rows sorted by shape, q_offsets (B + 1);
    keys a list of K (rows, offsets) pairs, one per neighbour rank (``get_neighbors``, csn_utils.py:114-130: key batch i holds
    the i-th neighbour of every query shape).  Returns (N, out_channels), or with ``return_ssa`` the SSA rows (N, d_model)."""

    def __init__(self, d_model: int, n_head: int, out_channels: int, k_neighbors: int, dropout: float = 0.1,
                 backbone_channels: Optional[int] = None, bn_momentum: float = 0.02):
        super().__init__()
        if d_model not in LN_WIDTHS:
            raise ValueError(f"d_model {d_model} is not supported: the LayerNorm epilogues are built for d_model in {LN_WIDTHS}")
        self.d_model, self.n_head, self.k_neighbors = d_model, n_head, k_neighbors
        self.MHA = MultiHeadAttention(n_head, d_model, d_model // n_head, d_model // n_head, dropout=dropout,
                                      return_attention=False)
        self.output = nn.Linear(d_model * 2, out_channels, bias=True)
        if k_neighbors > 0:
            self.linear_q = nn.Linear(d_model, d_model, bias=False)
            self.linear_k = nn.Linear(d_model, d_model, bias=False)
            self.sim = ScaledDotProduct(d_model ** 0.5)
        self.backbone_channels = backbone_channels
        if backbone_channels is not None:
            self.fc_layer = BackboneFC(backbone_channels, d_model, bn_momentum=bn_momentum)

    @staticmethod
    def cosine_similarity(q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
        """hrnet.py:472-490 (see the module-level ``cosine_similarity``)."""
        return cosine_similarity(q, k)

    def _attend(self, qs: List[torch.Tensor], ks: List[torch.Tensor]) -> torch.Tensor:
        """One varlen launch chain for the evaluations MHA(qs[e], ks[e], ks[e]): xhat (E, C, round-up-4(max query count))."""
        dev, C = qs[0].device, self.d_model
        nq, nk = [int(t.shape[0]) for t in qs], [int(t.shape[0]) for t in ks]
        Lq, Lk = max(nq), max(nk)
        pad = lambda ts, n: torch.stack([F.pad(t, (0, 0, 0, n - t.shape[0])) for t in ts])
        xq, xk = pad(qs, Lq), pad(ks, Lk)
        q_lens = torch.tensor([_up(n, 4) for n in nq], dtype=torch.int32).to(dev)
        k_lens = torch.tensor(nk, dtype=torch.int32).to(dev)
        m = self.MHA
        p_attn, p_fc = (m.attention.dropout.p, m.dropout.p) if self.training else (0.0, 0.0)
        ws = m.kernel_weights()
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in (xq, xk) + ws)
        xhat, _ = _CrossMHA.apply(xq, xk, xk, *ws, m.n_head, m.d_head, float(p_attn), float(p_fc), False, keep, q_lens, k_lens,
                                  m._temperature())
        return xhat

    def forward(self, q: torch.Tensor, q_offsets, keys: Optional[Sequence[Ragged]] = None, return_ssa: bool = False):
        if not q.is_cuda:
            raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        c_rows = self.d_model if self.backbone_channels is None else self.backbone_channels
        if q.dim() != 2 or q.shape[1] != c_rows:
            raise ValueError(f"queries must be (N, {c_rows}) rows")
        K = 0 if (keys is None or return_ssa) else len(keys)
        if K > 0 and self.k_neighbors == 0:
            raise ValueError("this head was built with k_neighbors = 0 (no linear_q / linear_k): it takes no key batches")
        if K > 8 - 1:
            raise ValueError("at most 7 neighbours (k1 = K + 1 <= 8)")
        dev = q.device
        q = q.float()
        qo = _host_offsets(q_offsets, q.shape[0])
        B = len(qo) - 1
        if self.backbone_channels is not None:
            # fc_layer on the query batch, then on key batch 0 .. K-1 (hrnet.py:439, :451): the order of the running statistics
            for rows, offs in (keys or [])[:K]:
                if not rows.is_cuda:
                    raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
                if rows.dim() != 2 or rows.shape[1] != c_rows:
                    raise ValueError(f"key batches must be (N, {c_rows}) rows")
                _host_offsets(offs, rows.shape[0])
            q = self.fc_layer(q)
            keys = [(self.fc_layer(rows), offs) for rows, offs in (keys or [])[:K]]
        q_shapes = [q[a:b] for a, b in zip(qo, qo[1:])]
        k_shapes = []
        for rows, offs in (keys or [])[:K]:
            if not rows.is_cuda:
                raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
            ko = _host_offsets(offs, rows.shape[0])
            if len(ko) - 1 != B:
                raise ValueError(f"every key batch needs one shape per query shape ({B})")
            rows = rows.float()
            k_shapes.append([rows[a:b] for a, b in zip(ko, ko[1:])])
        # evaluation order: S_b, T_{i,b}, X_{i,b} (module docstring)
        qs = q_shapes + [t for ks in k_shapes for t in ks] + q_shapes * K
        kv = q_shapes + [t for ks in k_shapes for t in ks] * 2
        xhat = self._attend(qs, kv)
        counts = [int(t.shape[0]) for t in qs]
        plan = {"B": B, "K": K, "ssa_only": return_ssa, "cross_first": B + K * B, "offsets": _int32_pair(qo, dev),
                "counts": _int32_pair(counts, dev), "sim": getattr(self, "sim", None)}
        wq = self.linear_q.weight if K > 0 else self.MHA.norm.weight.new_empty(0)
        wk = self.linear_k.weight if K > 0 else wq
        out = _RaggedHead.apply(xhat, self.MHA.norm.weight, self.MHA.norm.bias, wq, wk, q, plan)
        if return_ssa:
            return out
        return F.linear(out, self.output.weight, self.output.bias)                              # hrnet.py:423


def cosine_similarity(q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """hrnet.py:472-490: mean over q's rows of the max over k's rows of the cosine, a 0-dim tensor — through the ragged
    retrieval kernel (no n x m matrix).  Rows are normalised with max(|x|, 1e-12) where the reference divides by |x|: the two
    differ only for an all-zero row (the reference gives nan there)."""
    return retrieval_measure_ragged(q, [0, q.shape[0]], k, [0, k.shape[0]])[0, 0]


# ------------------------------------------------------------------------------------------------------
# shape graph
# ------------------------------------------------------------------------------------------------------
def shape_ssa(head: SimCSNHead, shapes: Sequence[torch.Tensor], max_rows: int = 1 << 15) -> Tuple[torch.Tensor, List[int]]:
    """SSA rows of every shape (``head(.., return_ssa=True)``, no grad) in varlen chunks of at most ``max_rows`` rows (at least
    one shape per chunk): packed rows (N, d_model) and their offsets."""
    outs, off = [], [0]
    with torch.no_grad():
        i = 0
        while i < len(shapes):
            j, rows = i, 0
            while j < len(shapes) and (j == i or rows + shapes[j].shape[0] <= max_rows):
                rows += shapes[j].shape[0]
                j += 1
            chunk = [s.float() for s in shapes[i:j]]
            co = [0]
            for s in chunk:
                co.append(co[-1] + s.shape[0])
            outs.append(head(torch.cat(chunk), co, return_ssa=True))
            off += [off[-1] + c for c in co[1:]]
            i = j
    return torch.cat(outs), off


def construct_shape_graph(head: SimCSNHead, query_shapes: Sequence[torch.Tensor], key_shapes: Optional[Sequence[torch.Tensor]] = None,
                          K: int = 1, random_pairs: bool = False, rng: Optional[np.random.Generator] = None,
                          max_rows: int = 1 << 15, screen: Optional[bool] = None) -> List[Tuple[int, List[int]]]:
    """csn_utils.py:11-111 on per-shape backbone features ``query_shapes[i]`` (n_i, d_model) (device tensors): the K
    neighbours of every query shape among ``key_shapes`` (None: among the queries themselves, never the query).  Returns
    ``[(q_idx, [neighbours])]``.  ``random_pairs``: the random branch (:31-43) drawn from ``rng`` (a numpy Generator).
    Similarity branch (:44-97): the SSA of every shape (chunked varlen calls, no grad, the head's current train / eval mode as
    in the reference), the ragged retrieval measure of every (query, key) pair, and the top-K rule of :91-96.
    ``screen``: True scores only the pairs an fp16 screen cannot rule out (``topk_retrieval_ragged``: the same neighbours, the
    fp32 measure alone ranks), False every pair, None follows ``tuning.current().retrieval_screen`` (off by default)."""
    if K < 1:
        raise ValueError("K must be >= 1 (csn_utils.py:16)")
    is_same = key_shapes is None
    n_key = len(query_shapes) if is_same else len(key_shapes)
    if random_pairs:
        if rng is None:
            raise ValueError("random_pairs needs an explicit numpy Generator (rng)")
        return random_neighbors(len(query_shapes), n_key, K, is_same, rng)
    q_rows, q_off = shape_ssa(head, query_shapes, max_rows)
    k_rows, k_off = (q_rows, q_off) if is_same else shape_ssa(head, key_shapes, max_rows)
    with torch.no_grad():
        if tuning.current().retrieval_screen if screen is None else screen:
            return topk_retrieval_ragged(q_rows, q_off, k_rows, k_off, K, is_same)[0]
        sim = retrieval_measure_ragged(q_rows, q_off, k_rows, k_off)
    return topk_neighbors(sim.cpu(), K, is_same)
