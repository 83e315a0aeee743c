"""The KV_SAME instance of the d = 256 two-plane attention backward (csrc/attn_bf16x3.hip; CSN_DEV_KV_SAME, ``tuning.kv_same``):
where k and v are the same tile planes (folded projections) the no-planes dQ kernel requests every 32-key tile once and commits
the same registers into both LDS images.  Both instances run the same arithmetic on the same LDS contents, so everything here is
held BIT FOR BIT against the instance that requests a tile once per image (the key set to 0):

1. forward: att, lse and the kept scores, eval and train (attention dropout 0.1, the same seed).  The forward's own one-request
   instance was measured +-0 over the step and is not built: the key must not reach the forward at all;
2. dQ (probs_tiles = 3): G and delta, one grouped call (groups of K + 2 = 4 evaluations on a query slot, B = 2, K = 2) and the same
   evaluations colour by colour (accumulate = 1); G again with delta not requested (NULL);
3. the folded module step with ``kv_same`` on against off: loss and every parameter gradient;
4. dispatch: with k != v (the unfolded tile-plane step's operands) the instance is not chosen whatever the key says.

Shapes (keys per block T, blocks, points N): one tile exactly; a second tile of 4 keys; T = 128; T = 500 in 2 blocks (last tile 20
keys, a query tile of 116 rows); N = 1236 with T = 500 (a short last block of 236)."""
import numpy as np
import pytest
import torch

from oracle import csa_oracle as orc

pytestmark = pytest.mark.gpu

D = 256
SHAPES = [(32, 1, 32), (36, 1, 36), (128, 1, 128), (500, 2, 1000), (500, 3, 1236)]
SHAPE_IDS = ["one-tile", "tile-of-4-keys", "T128", "2x500", "short-last-block"]
B, K = 2, 2
K1 = K + 1
S = B * K1
SEED = 0x9e37_79b9_7f4a_7c15


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_dev_set(L.DEV_KV_SAME, 1)
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32)


def _plan():
    """MultiHeadAttention.plan("csa_train"): the query shape's slot b * K1 serves K1 mixed evaluations and the pooled one"""
    from csn_amd.functional import EvalPlan
    b, k = np.meshgrid(np.arange(B), np.arange(K1), indexing="ij")
    mix_q, mix_kv = (b * K1).reshape(-1), (b * K1 + k).reshape(-1)
    nbr = (b * K1 + k)[:, 1:].reshape(-1)
    own = np.arange(B) * K1
    plan = EvalPlan(np.concatenate((mix_q, nbr, own)), np.concatenate((mix_kv, nbr, own)), S, "cuda")
    assert int(np.diff(plan.q_group_off.cpu().numpy()).max()) == K + 2 and len(plan.dq_colors) == K + 2
    return plan


_cases = {}


def _case(L, T, nb, N):
    """seeded inputs of a shape, made once: x and its tile planes (csn_tile_planes_f32), queries, dO"""
    if (T, nb, N) not in _cases:
        lib = L.lib()
        rng = np.random.default_rng(7 * N + T)
        rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
        x, q, dctx = rnd(S, D, N), rnd(S, D, N) / 16, None
        ldp = nb * 1024
        planes = torch.zeros((S, D, ldp), dtype=torch.int16, device="cuda")
        L.check(lib.csn_tile_planes_f32(x.data_ptr(), D * N, N, planes.data_ptr(), D * ldp, ldp, S, D, N, T, _stream()), "planes")
        plan = _plan()
        dctx = rnd(plan.E, D, N)
        _cases[(T, nb, N)] = (x, q, planes, dctx, plan)
    return _cases[(T, nb, N)]


def _forward(L, key, q, k_ptr, v_ptr, kv_stride, ldp, plan, T, nb, N, p):
    lib = L.lib()
    E, Tp = plan.E, (T + 31) // 32 * 32
    assert lib.csn_dev_set(L.DEV_KV_SAME, key) >= 0 and lib.csn_dev_get(L.DEV_KV_SAME) == key
    att = torch.full((E, D, N), float("nan"), device="cuda")
    lse = torch.full((E, 1, nb * T), float("nan"), device="cuda")
    sc = torch.full((E, 1, nb, T, Tp), float("nan"), device="cuda")
    L.check(lib.csn_block_attn_fwd_grouped_f32(q.data_ptr(), k_ptr, v_ptr, D * N, kv_stride, plan.q_slots.data_ptr(),
                                               plan.kv_slots.data_ptr(), N, att.data_ptr(), D * N, sc.data_ptr(), lse.data_ptr(), E, 1, D,
                                               T, nb, Tp, 8.0, p, SEED + T, 1, ldp, plan.q_group_items.data_ptr(),
                                               plan.q_group_off.data_ptr(), plan.n_q_groups, _stream()), "forward")
    torch.cuda.synchronize()
    return att, lse, sc


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "train"])
@pytest.mark.parametrize("T,nb,N", SHAPES, ids=SHAPE_IDS)
def test_forward_bit_for_bit(L, T, nb, N, p):
    """k == v in the forward, the key off and on: the same bits (the forward has one instance; the key belongs to the dQ call)."""
    L.check(L.lib().csn_set_math_mode(1))
    x, q, planes, _, plan = _case(L, T, nb, N)
    ldp = nb * 1024
    runs = [_forward(L, key, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, p) for key in (0, 1)]
    for name, a, b in zip(("att", "lse", "scores"), *runs):
        assert torch.equal(_bits(a), _bits(b)), name
    att, lse, _ = runs[1]
    assert torch.isfinite(att).all() and torch.isfinite(lse[..., :N]).all()
    if p == 0.0:
        # the instance computes attention at all: float64 softmax(q^T x) x^T of the first evaluation's first block
        t0 = min(T, N)
        pr = torch.softmax(q[0, :, :t0].double().t() @ x[0, :, :t0].double(), dim=-1)
        ref = (pr @ x[0, :, :t0].double().t()).t()
        assert (att[0, :, :t0].double() - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "train"])
@pytest.mark.parametrize("T,nb,N", SHAPES, ids=SHAPE_IDS)
def test_dq_bit_for_bit(L, T, nb, N, p):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    _, q, planes, dctx, plan = _case(L, T, nb, N)
    ldp, E, Tp = nb * 1024, plan.E, (T + 31) // 32 * 32
    assert lib.csn_attn_bwd_dq_no_planes_available(D, T)
    att, lse, sc = _forward(L, 0, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, p)

    def dq_call(key, grouped, want_delta=True):
        assert lib.csn_dev_set(L.DEV_KV_SAME, key) >= 0
        scb = sc.clone()
        delta = torch.full((E, 1, nb * T), float("nan"), device="cuda") if want_delta else None
        dq = torch.full((S, D, N), float("nan"), device="cuda")
        if grouped:
            launches = [(0, plan.q_group_items, E, plan.q_group_off, plan.n_q_groups)]
        else:
            launches = [(0 if ci == 0 else 1, ids, ids.numel(), None, 0) for ci, ids in enumerate(plan.dq_colors)]
        for accumulate, ids, n_ids, off, n_groups in launches:
            L.check(lib.csn_block_attn_bwd_dq_f32(dctx.data_ptr(), att.data_ptr(), D * N, planes.data_ptr(), planes.data_ptr(), D * ldp,
                                                  plan.kv_slots.data_ptr(), N, scb.data_ptr(), None, lse.data_ptr(),
                                                  delta.data_ptr() if want_delta else None, dq.data_ptr(), D * N,
                                                  plan.q_slots.data_ptr(), accumulate, ids.data_ptr(), n_ids, 1, D, T, nb, Tp, p,
                                                  SEED + T, 0, 0, 1, ldp, 3, off.data_ptr() if off is not None else None, n_groups,
                                                  _stream()), "dq")
        torch.cuda.synchronize()
        assert torch.equal(_bits(scb), _bits(sc)), "the scores were touched"
        return dq, delta

    for grouped in (True, False):
        dq0, delta0 = dq_call(0, grouped)
        dq1, delta1 = dq_call(1, grouped)
        assert torch.equal(_bits(dq1), _bits(dq0)), ("dQ", grouped)
        assert torch.equal(_bits(delta1), _bits(delta0)), ("delta", grouped)
        written = sorted(set(plan.q_slots.tolist()))
        assert torch.isfinite(dq1[written]).all() and torch.isfinite(delta1[..., :N]).all()
        unwritten = [s for s in range(S) if s not in written]
        assert torch.isnan(dq1[unwritten]).all()
        if grouped:
            dq2, _ = dq_call(1, True, want_delta=False)                  # delta not requested (NULL): the same dQ
            assert torch.equal(_bits(dq2), _bits(dq0)), "dQ without delta"


def test_not_chosen_when_k_is_not_v(L):
    """K and V planes of a [K | V] projection: were the instance chosen, the value image would hold K — so results that equal the
    key-off run show it was not; the key itself reads back what was set, and refuses other bits."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    T, nb, N = 500, 2, 1000
    x, q, _, dctx, plan = _case(L, T, nb, N)
    ldp, E, Tp = nb * 1024, plan.E, (T + 31) // 32 * 32
    w = torch.from_numpy(np.random.default_rng(5).standard_normal((2 * D, D)).astype(np.float32) / 16).cuda()
    kv = torch.zeros((S, 2 * D, ldp), dtype=torch.int16, device="cuda")
    L.check(lib.csn_project_f32(x.data_ptr(), D * N, N, w.data_ptr(), 2 * D, D, kv.data_ptr(), 2 * D * ldp, ldp, S, N, 0, 1.0, 2, T,
                                _stream()), "K | V")
    k_ptr, v_ptr = kv.data_ptr(), kv.data_ptr() + 2 * D * ldp
    assert lib.csn_dev_get(L.DEV_KV_SAME) == 1
    assert lib.csn_dev_set(L.DEV_KV_SAME, 2) == -1 and lib.csn_dev_set(L.DEV_KV_SAME, -1) == -1 and lib.csn_dev_get(L.DEV_KV_SAME) == 1
    runs = {}
    for key in (0, 1):
        att, lse, sc = _forward(L, key, q, k_ptr, v_ptr, 2 * D * ldp, ldp, plan, T, nb, N, 0.1)
        dq = torch.full((S, D, N), float("nan"), device="cuda")
        delta = torch.full((E, 1, nb * T), float("nan"), device="cuda")
        L.check(lib.csn_block_attn_bwd_dq_f32(dctx.data_ptr(), att.data_ptr(), D * N, k_ptr, v_ptr, 2 * D * ldp, plan.kv_slots.data_ptr(),
                                              N, sc.data_ptr(), None, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), D * N,
                                              plan.q_slots.data_ptr(), 0, plan.q_group_items.data_ptr(), E, 1, D, T, nb, Tp, 0.1,
                                              SEED + T, 0, 0, 1, ldp, 3, plan.q_group_off.data_ptr(), plan.n_q_groups, _stream()), "dq")
        torch.cuda.synchronize()
        assert lib.csn_dev_get(L.DEV_KV_SAME) == key
        runs[key] = (att, lse, sc, dq, delta)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(b))
    # ... and K != V matters here: the same call on the K planes as both gives another result
    att_kk = _forward(L, 0, q, k_ptr, k_ptr, 2 * D * ldp, ldp, plan, T, nb, N, 0.1)[0]
    assert not torch.equal(_bits(att_kk), _bits(runs[0][0]))


@pytest.mark.parametrize("N", [1500, 1236], ids=["3x500", "short-last-block"])
def test_module_step_bit_for_bit(L, N):
    """The folded CrossShapeAt training step at the geometry of tests/test_gpu_folded.py: the switch on against off."""
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    L.check(L.lib().csn_set_math_mode(1))
    n_cls, T, n_blocks = 7, 500, 3
    geo = dict(block=T, n_blocks=n_blocks if N == T * n_blocks else None)
    p, x, nb, lab = orc.conditioned_csa_case(np.random.default_rng(4004 + N), B, K, 1, n_cls, 4.0, 2.0, 1.0, n_points=N)
    runs = {}
    for on in (False, True):
        model = get_model("csa", n_cls, 1, K, **geo)
        model.load_state_dict(p, strict=False)
        model = model.cuda().train(True)
        calls = []
        L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
        try:
            torch.manual_seed(9)
            with tuning.override(kv_same=on):
                loss = orc.masked_ce_loss(model(x.cuda(), "train", nb.cuda()), lab.cuda())
                loss.backward()
        finally:
            L.set_call_hook(None)
        assert "csn_fold_weights_f32" in calls, "the step did not fold"
        assert calls.count("csn_block_attn_bwd_dq_f32") == 1 and "csn_block_attn_bwd_dkv_f32" not in calls
        assert L.lib().csn_dev_get(L.DEV_KV_SAME) == int(on)
        runs[on] = (loss.detach(), {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    assert torch.equal(_bits(runs[True][0]), _bits(runs[False][0])), "loss"
    assert len(runs[True][1]) == len(runs[False][1]) == 11
    for n, g in runs[True][1].items():
        assert torch.equal(_bits(g), _bits(runs[False][1][n])), n
