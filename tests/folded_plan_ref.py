"""float64 restatement of ``MultiHeadAttention.evaluate`` for an arbitrary evaluation plan — test infrastructure
(tests/test_cpu_folded_plan_ref.py holds it to the oracle, tests/test_gpu_folded_plans.py holds the kernels to it).

Plain torch autograd on the CPU.  For every evaluation e = (query slot, key/value slot) and every block of T points
(MID-FC/csa_models.py:81-125, the last block short when T does not divide N):

    P    = softmax((x_q W_q^T / t) (x_k W_k^T)^T)         the UNFOLDED association: Q, K and V are formed
    P    = P * attention mask / (1 - p)                   (train mode)
    z    = (P (x_k W_v^T)) W_fc^T
    z    = z * fc mask / (1 - p)                          (train mode)
    xhat = layer_norm(z + x_q), eps 1e-6, no affine

and the results are xhat (E, C, N), sums = xhat.sum(-1) and the four weight gradients of L = <xhat, R> + <sums, Rs>.
``association="folded"`` runs the other association (M = W_k^T W_q / t, W_fv = W_fc W_v, attention on x itself), which is what
the folded step of csn_amd/functional.py computes — the CPU test holds the two to each other at 1e-12, nothing else uses it.

The masks are those of tests/dropout_ref.py under the two seeds the step draws through ``CF.draw_seeds``; the plans come from
``MultiHeadAttention.plan`` of a module built on the CPU, the inputs from ``oracle.conditioned_csa_case`` (the inputs of the
project's 1e-4 contract)."""
import numpy as np
import torch

from oracle import csa_oracle as orc
from tests import dropout_ref as dr

B, K, C, N_CLS = 2, 2, 256, 7
K1 = K + 1
P_DROP = 0.1
STEP_SEED = 9                       # torch.manual_seed of a step (as tests/test_gpu_folded.py::_module_step)
TENSORS = ("xhat", "sums", "dw_q", "dw_k", "dw_v", "dw_fc")

# (T, N): one key tile | three blocks, a second tile of 4 keys, a short last block of 28 | one full query tile | a 20-key last
# tile and a short last block of 236
SMALL = ((32, 32), (36, 100), (128, 128))
BIG = (500, 736)
IRREGULAR = ([0, 2, 0, 3, 0, 2, 0], [0, 2, 1, 3, 2, 0, 3], 4)     # of tests/test_gpu_grouped_fwd.py: slot 1 never queried, groups 4, 2, 1
PLANS = ("self", "cross", "csa", "csa_train", "self2", "csa_cross", "cross_only", "irregular")
PLAN_K1 = {"self": 1, "cross": 1, "self2": 1}                    # the K1 argument of MultiHeadAttention.plan (others: K + 1)


def gpu_cases():
    """every (plan, T, N, train) tests/test_gpu_folded_plans.py runs against this file"""
    out = [(plan, T, N, train) for plan in PLANS for T, N in SMALL for train in (False, True)]
    return out + [(plan, *BIG, True) for plan in ("csa_train", "cross_only")]


def make_plan(att, kind, dev):
    """The EvalPlan of ``kind`` on ``dev`` from the module's own table (the irregular one from its slot lists)."""
    from csn_amd import functional as CF
    if kind == "irregular":
        q, kv, S = IRREGULAR
        return CF.EvalPlan(np.array(q), np.array(kv), S, dev)
    return att.plan(kind, B, PLAN_K1.get(kind, K1), dev)


_table = {}


def plan_table():
    """{kind: (q_slots, kv_slots, n_slots)} as MultiHeadAttention.plan gives them (nothing restated by hand)."""
    if not _table:
        from csn_amd.csa_models import MultiHeadAttention
        att = MultiHeadAttention(1, C, C, C)
        for kind in PLANS:
            pl = make_plan(att, kind, "cpu")
            _table[kind] = (pl.q_slots.tolist(), pl.kv_slots.tolist(), pl.S)
    return _table


def step_seeds(seed=STEP_SEED):
    """(attention seed, fc seed) a step draws after torch.manual_seed(seed): CF.draw_seeds(2) on torch's CPU generator"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2 ** 62, (2,), generator=g).tolist()


_cases = {}


def case(kind, T, N):
    """Weights, slots and cotangents of one (plan, geometry): the parameters and features of orc.conditioned_csa_case, the slots
    the first S maps of its neighbour stack (slot b*K1 + k = neighbour k of shape b, k = 0 the shape itself), R and Rs standard
    normal.  Cached; nobody writes to the tensors."""
    key = (kind, T, N)
    if key not in _cases:
        q, kv, S = plan_table()[kind]
        rng = np.random.default_rng(8800 + 7 * T + N)
        p, x, nb, lab = orc.conditioned_csa_case(rng, B, K, 1, N_CLS, 4.0, 2.0, 1.0, n_points=N)
        E = len(q)
        _cases[key] = dict(
            kind=kind, T=T, N=N, n_blocks=(N + T - 1) // T, S=S, E=E, q_slots=q, kv_slots=kv,
            x_all=nb.squeeze(-1).reshape(B * K1, C, N)[:S].contiguous(),
            w={n: p[f"attention.{n}.weight"] for n in ("w_qs", "w_ks", "w_vs", "fc")},
            R=torch.from_numpy(rng.standard_normal((E, C, N)).astype(np.float32)),
            Rs=torch.from_numpy(rng.standard_normal((E, C)).astype(np.float32)))
    return _cases[key]


def masks(E, T, N, seeds, p=P_DROP):
    """(attention mask [e][block][query][key], fc mask [e][c][n]) as bool tensors: tests/dropout_ref.py, the attention mask
    transposed to [query][key] as tests/test_gpu_folded.py::_masked_oracle does"""
    n_blocks, Tp = (N + T - 1) // T, (T + 31) // 32 * 32
    am = torch.from_numpy(dr.attention_mask(E, 1, n_blocks, T, Tp, seeds[0], p))[:, 0].transpose(-1, -2)
    fm = torch.from_numpy(dr.fc_mask(E, C, N, seeds[1], p))
    return am, fm


def evaluate_ref(x_all, w_q, w_k, w_v, w_fc, q_slots, kv_slots, T, R, Rs, am=None, fm=None, p=0.0, dtype=torch.float64,
                 association="unfolded"):
    """-> {xhat (E, C, N), sums (E, C), dw_q, dw_k, dw_v, dw_fc} in ``dtype``; am / fm None: eval mode."""
    w_q, w_k, w_v, w_fc = (w.detach().to(dtype).clone().requires_grad_(True) for w in (w_q, w_k, w_v, w_fc))
    x = x_all.to(dtype)
    N = x.shape[2]
    t = float(w_q.shape[0]) ** 0.5                           # one head of width d_k (MID-FC/csa_models.py:54)
    xq = x[list(q_slots)].permute(0, 2, 1)                   # (E, N, C)
    xk = x[list(kv_slots)].permute(0, 2, 1)
    if association == "folded":
        m, w_fv = w_k.t() @ w_q / t, w_fc @ w_v
    outs = []
    for blk in range((N + T - 1) // T):
        sl = slice(blk * T, min(N, (blk + 1) * T))
        t_b = sl.stop - sl.start
        a, b_ = xq[:, sl], xk[:, sl]
        if association == "folded":
            scores = (a @ m.t()) @ b_.transpose(1, 2)
        else:
            scores = (a @ w_q.t() / t) @ (b_ @ w_k.t()).transpose(1, 2)
        pr = torch.softmax(scores, dim=-1)
        if am is not None:
            pr = pr * am[:, blk, :t_b, :t_b].to(dtype) / (1.0 - p)
        z = (pr @ b_) @ w_fv.t() if association == "folded" else (pr @ (b_ @ w_v.t())) @ w_fc.t()
        if fm is not None:
            z = z * fm[:, :, sl].permute(0, 2, 1).to(dtype) / (1.0 - p)
        outs.append(torch.nn.functional.layer_norm(z + a, (a.shape[-1],), None, None, 1e-6))
    xhat = torch.cat(outs, dim=1).permute(0, 2, 1)           # (E, C, N)
    sums = xhat.sum(-1)
    loss = (xhat * R.to(dtype)).sum() + (sums * Rs.to(dtype)).sum()
    grads = torch.autograd.grad(loss, (w_q, w_k, w_v, w_fc))
    return dict(zip(TENSORS, (xhat.detach(), sums.detach()) + tuple(grads)))


def reference(c, train, seeds=None, dtype=torch.float64, association="unfolded"):
    """evaluate_ref on a ``case``; train: with the p = 0.1 masks of ``seeds`` (None: step_seeds())"""
    am = fm = None
    if train:
        am, fm = masks(c["E"], c["T"], c["N"], step_seeds() if seeds is None else seeds)
    w = c["w"]
    return evaluate_ref(c["x_all"], w["w_qs"], w["w_ks"], w["w_vs"], w["fc"], c["q_slots"], c["kv_slots"], c["T"], c["R"], c["Rs"],
                        am, fm, P_DROP if train else 0.0, dtype, association)


def ratios(got, ref):
    """{tensor: max |got - ref| / max |ref|}"""
    return {n: (got[n].double() - ref[n].double()).abs().max().item() / ref[n].double().abs().max().item() for n in TENSORS}
