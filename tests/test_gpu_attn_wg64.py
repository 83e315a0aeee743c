"""The 64-query instance of the d = 256 bf16x3 attention backward (csrc/attn_bf16x3.hip WG64; CSN_DEV_ATTN_WG64, ``tuning.wg64``):
where k and v are the same tile planes (folded projections) the no-planes dQ runs as four waves and 64 queries per work-group on
ONE LDS tile image (csrc/attn_tile_image.h), two work-groups per CU.  The arithmetic per query row and its order are those of
the eight-wave instance, so everything here is held BIT FOR BIT against the same call with the key 0:

1. forward: att, lse and the kept scores, eval and train (attention dropout 0.1, one seed), through
   csn_block_attn_fwd_grouped_f32 and csn_block_attn_fwd_f32.  The forward's own 64-query instance did not clear the step A/B's
   noise bar and is not built (DESIGN.md §4m "Two work-groups per CU"): the key must not reach the forward at all;
2. dQ (probs_tiles = 3): G with delta requested and with delta NULL; one grouped call, and the same evaluations colour by colour
   (accumulate = 1);
3. the folded module step with ``tuning.wg64`` on against off: the loss and every parameter gradient, train mode;
4. dispatch: with k != v (the unfolded step's tile-plane operands), at d = 128, in math mode 2 and on a forward that keeps no
   scores (a recomputing flow's) the form is not chosen whatever the key says — the bits equal the key-0 call AND the library's
   launch counter (CSN_DEV_ATTN_WG64_LAUNCHES) stands still; where the form is chosen the counter moves by one per launch.
   (At d = 256 in bf16x3 no recomputing backward exists — three tile images do not fit a CU — so that flow is its forward.)

Shapes (keys per block T, blocks, points N): half a work-group; a second tile of 4 keys; exactly one work-group; a second
work-group of 4 rows; what was one work-group is now two; 132; T = 500 in 2 blocks (8 query tiles, the last of 52 rows, last key
tile of 20 keys); N = 1236 (a short last block of 236).  T = 35 (T & 3 != 0): the tile-plane entry points refuse such a block
(CSN_E_ALIGN — keys are masked one by one only on fp32 K / V maps, which the form never takes), so that case holds what CAN be
held: the refusal is the same under both keys, and the cross-length forward on fp32 maps with 35 keys gives the key-0 bits
without a launch of the form."""
import numpy as np
import pytest
import torch

from oracle import csa_oracle as orc

pytestmark = pytest.mark.gpu

D = 256
SHAPES = [(32, 1, 32), (36, 1, 36), (64, 1, 64), (68, 1, 68), (128, 1, 128), (132, 1, 132), (500, 2, 1000), (500, 3, 1236)]
SHAPE_IDS = ["half-group", "tile-of-4-keys", "one-group", "group-of-4-rows", "two-groups", "T132", "2x500", "short-last-block"]
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
    L.lib().csn_dev_set(L.DEV_ATTN_WG64, 1)
    L.lib().csn_dev_set(L.DEV_KV_SAME, 1)
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32)


def _count(L):
    return L.lib().csn_dev_get(L.DEV_ATTN_WG64_LAUNCHES)


def _set(L, key):
    lib = L.lib()
    assert lib.csn_dev_set(L.DEV_ATTN_WG64, key) >= 0 and lib.csn_dev_get(L.DEV_ATTN_WG64) == key


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


def _case(L, T, nb, N, d=D):
    """seeded inputs of a shape, made once: x and its tile planes (csn_tile_planes_f32), queries, dO"""
    if (T, nb, N, d) not in _cases:
        lib = L.lib()
        rng = np.random.default_rng(7 * N + T + d)
        rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
        x, q = rnd(S, d, N), rnd(S, d, N) / 16
        ldp = nb * 1024
        planes = torch.zeros((S, d, ldp), dtype=torch.int16, device="cuda")
        L.check(lib.csn_tile_planes_f32(x.data_ptr(), d * N, N, planes.data_ptr(), d * ldp, ldp, S, d, N, T, _stream()), "planes")
        plan = _plan()
        dctx = rnd(plan.E, d, N)
        _cases[(T, nb, N, d)] = (x, q, planes, dctx, plan)
    return _cases[(T, nb, N, d)]


def _forward(L, key, q, k_ptr, v_ptr, kv_stride, ldp, plan, T, nb, N, p, grouped=True, d=D, keep=True):
    lib = L.lib()
    E, Tp = plan.E, (T + 31) // 32 * 32
    _set(L, key)
    att = torch.full((E, d, N), float("nan"), device="cuda")
    lse = torch.full((E, 1, nb * T), float("nan"), device="cuda")
    sc = torch.full((E, 1, nb, T, Tp), float("nan"), device="cuda")
    head = (q.data_ptr(), k_ptr, v_ptr, d * N, kv_stride, plan.q_slots.data_ptr(), plan.kv_slots.data_ptr(), N, att.data_ptr(), d * N,
            sc.data_ptr() if keep else None, lse.data_ptr(), E, 1, d, T, nb, Tp, 8.0, p, SEED + T, 1, ldp)
    if grouped:
        rc = lib.csn_block_attn_fwd_grouped_f32(*head, plan.q_group_items.data_ptr(), plan.q_group_off.data_ptr(), plan.n_q_groups,
                                                _stream())
    else:
        rc = lib.csn_block_attn_fwd_f32(*head, _stream())
    L.check(rc, "forward")
    torch.cuda.synchronize()
    return att, lse, sc


def _dq(L, key, planes_k, planes_v, kv_stride, ldp, plan, T, nb, N, p, att, lse, sc, dctx, grouped=True, want_delta=True, d=D):
    lib = L.lib()
    E, Tp = plan.E, (T + 31) // 32 * 32
    _set(L, key)
    scb = sc.clone()
    delta = torch.full((E, 1, nb * T), float("nan"), device="cuda") if want_delta else None
    dq = torch.full((S, d, N), float("nan"), device="cuda")
    if grouped:
        launches = [(0, plan.q_group_items, E, plan.q_group_off, plan.n_q_groups)]
    else:
        launches = [(0 if ci == 0 else 1, ids, ids.numel(), None, 0) for ci, ids in enumerate(plan.dq_colors)]
    for accumulate, ids, n_ids, off, n_groups in launches:
        L.check(lib.csn_block_attn_bwd_dq_f32(dctx.data_ptr(), att.data_ptr(), d * N, planes_k, planes_v, kv_stride,
                                              plan.kv_slots.data_ptr(), N, scb.data_ptr(), None, lse.data_ptr(),
                                              delta.data_ptr() if want_delta else None, dq.data_ptr(), d * N,
                                              plan.q_slots.data_ptr(), accumulate, ids.data_ptr(), n_ids, 1, d, T, nb, Tp, p,
                                              SEED + T, 0, 0, 1, ldp, 3, off.data_ptr() if off is not None else None, n_groups,
                                              _stream()), "dq")
    torch.cuda.synchronize()
    assert torch.equal(_bits(scb), _bits(sc)), "the scores were touched"
    return dq, delta, len(launches)


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "train"])
@pytest.mark.parametrize("T,nb,N", SHAPES, ids=SHAPE_IDS)
def test_forward_bit_for_bit(L, T, nb, N, p):
    L.check(L.lib().csn_set_math_mode(1))
    x, q, planes, _, plan = _case(L, T, nb, N)
    ldp = nb * 1024
    for grouped in (True, False):
        n0 = _count(L)
        ref = _forward(L, 0, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, p, grouped)
        new = _forward(L, 1, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, p, grouped)
        assert _count(L) == n0, "the key reached the forward"
        for name, a, b in zip(("att", "lse", "scores"), new, ref):
            assert torch.equal(_bits(a), _bits(b)), (name, grouped)
    att, lse, _ = ref
    assert torch.isfinite(att).all() and torch.isfinite(lse[..., :N]).all()
    if p == 0.0:
        # the instances compute attention at all: float64 softmax(q^T x) x^T of the first evaluation's first block
        t0 = min(T, N)
        pr = torch.softmax(q[0, :, :t0].double().t() @ x[0, :, :t0].double(), dim=-1)
        want = (pr @ x[0, :, :t0].double().t()).t()
        assert (att[0, :, :t0].double() - want).abs().max().item() <= 2e-4 * want.abs().max().item()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "train"])
@pytest.mark.parametrize("T,nb,N", SHAPES, ids=SHAPE_IDS)
def test_dq_bit_for_bit(L, T, nb, N, p):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    _, q, planes, dctx, plan = _case(L, T, nb, N)
    ldp = nb * 1024
    assert lib.csn_attn_bwd_dq_no_planes_available(D, T)
    att, lse, sc = _forward(L, 0, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, p)
    pp = planes.data_ptr()
    for grouped in (True, False):
        n0 = _count(L)
        dq0, delta0, _ = _dq(L, 0, pp, pp, D * ldp, ldp, plan, T, nb, N, p, att, lse, sc, dctx, grouped)
        assert _count(L) == n0, "key 0 launched the form"
        dq1, delta1, n_launch = _dq(L, 1, pp, pp, D * ldp, ldp, plan, T, nb, N, p, att, lse, sc, dctx, grouped)
        assert _count(L) == n0 + n_launch, "the form was not launched"
        assert torch.equal(_bits(dq1), _bits(dq0)), ("dQ", grouped)
        assert torch.equal(_bits(delta1), _bits(delta0)), ("delta", grouped)
        written = sorted(set(plan.q_slots.tolist()))
        assert torch.isfinite(dq1[written]).all() and torch.isfinite(delta1[..., :N]).all()
        unwritten = [s for s in range(S) if s not in written]
        assert torch.isnan(dq1[unwritten]).all()
        dq2, _, _ = _dq(L, 1, pp, pp, D * ldp, ldp, plan, T, nb, N, p, att, lse, sc, dctx, grouped, want_delta=False)
        assert torch.equal(_bits(dq2), _bits(dq0)), ("dQ without delta", grouped)


def test_ragged_block_of_35_keys(L):
    """T = 35: no tile-plane call takes it (the same refusal under both keys); on fp32 maps the keys of the last 4-group are masked one
    by one by the eight-wave instance alone — the cross-length forward gives the key-0 bits and launches no 64-query instance."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    T = 35
    _, q, planes, _, plan = _case(L, 36, 1, 36)
    E, Tp = plan.E, 64
    att = torch.zeros((E, D, 36), device="cuda")
    lse = torch.zeros((E, 1, 36), device="cuda")
    sc = torch.zeros((E, 1, 1, 36, Tp), device="cuda")
    codes = []
    for key in (0, 1):
        _set(L, key)
        codes.append(lib.csn_block_attn_fwd_grouped_f32(q.data_ptr(), planes.data_ptr(), planes.data_ptr(), D * 36, D * 1024,
                                                        plan.q_slots.data_ptr(), plan.kv_slots.data_ptr(), 36, att.data_ptr(), D * 36,
                                                        sc.data_ptr(), lse.data_ptr(), E, 1, D, T, 1, Tp, 8.0, 0.1, SEED, 1, 1024,
                                                        plan.q_group_items.data_ptr(), plan.q_group_off.data_ptr(), plan.n_q_groups,
                                                        _stream()))
    assert codes[0] == codes[1] and codes[0] < 0, codes
    rng = np.random.default_rng(35)
    x = torch.from_numpy(rng.standard_normal((S, D, 36)).astype(np.float32)).cuda()
    n0, runs = _count(L), []
    for key in (0, 1):
        _set(L, key)
        o = torch.full((S, D, 36), float("nan"), device="cuda")
        ls = torch.full((S, 1, 36), float("nan"), device="cuda")
        s = torch.full((S, 1, 36, 36), float("nan"), device="cuda")
        L.check(lib.csn_cross_attn_fwd_f32(q.data_ptr(), x.data_ptr(), x.data_ptr(), D * 36, D * 36, 36, 36, o.data_ptr(), D * 36,
                                           s.data_ptr(), ls.data_ptr(), S, 1, D, 36, T, 36, 8.0, 0.1, SEED, _stream()), "cross forward")
        torch.cuda.synchronize()
        runs.append((o, ls, s[..., :T]))
    assert _count(L) == n0
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all()


def test_not_chosen_elsewhere(L):
    """k != v, d = 128, math mode 2, a forward that keeps no scores: the eight-wave instances, whatever the key says."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    assert lib.csn_dev_get(L.DEV_ATTN_WG64) == 1
    assert lib.csn_dev_set(L.DEV_ATTN_WG64, 2) == -1 and lib.csn_dev_set(L.DEV_ATTN_WG64, -1) == -1
    assert lib.csn_dev_set(L.DEV_ATTN_WG64_LAUNCHES, 0) == -1 and lib.csn_dev_get(L.DEV_ATTN_WG64) == 1
    T, nb, N = 500, 2, 1000
    x, q, planes, dctx, plan = _case(L, T, nb, N)
    ldp = nb * 1024
    n0 = _count(L)

    def same(runs):
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(_bits(a), _bits(b))

    # k != v: the K and V planes of a [K | V] projection
    w = torch.from_numpy(np.random.default_rng(5).standard_normal((2 * D, D)).astype(np.float32) / 16).cuda()
    kv = torch.zeros((S, 2 * D, ldp), dtype=torch.int16, device="cuda")
    L.check(lib.csn_project_f32(x.data_ptr(), D * N, N, w.data_ptr(), 2 * D, D, kv.data_ptr(), 2 * D * ldp, ldp, S, N, 0, 1.0, 2, T,
                                _stream()), "K | V")
    k_ptr, v_ptr = kv.data_ptr(), kv.data_ptr() + 2 * D * ldp
    runs = {}
    for key in (0, 1):
        att, lse, sc = _forward(L, key, q, k_ptr, v_ptr, 2 * D * ldp, ldp, plan, T, nb, N, 0.1)
        dq, delta, _ = _dq(L, key, k_ptr, v_ptr, 2 * D * ldp, ldp, plan, T, nb, N, 0.1, att, lse, sc, dctx)
        runs[key] = (att, lse, sc, dq, delta)
    same(runs)
    assert torch.isfinite(runs[1][3][sorted(set(plan.q_slots.tolist()))]).all()
    # a forward that keeps no scores (inference, or the forward of a flow that recomputes them)
    same({key: _forward(L, key, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, 0.1, keep=False)[:2]
          for key in (0, 1)})
    # math mode 2 (one bf16 product; the planes' bytes read as one-plane tiles — any bytes do for a dispatch check)
    L.check(lib.csn_set_math_mode(2))
    same({key: _forward(L, key, q, planes.data_ptr(), planes.data_ptr(), D * ldp, ldp, plan, T, nb, N, 0.1) for key in (0, 1)})
    L.check(lib.csn_set_math_mode(1))
    # d = 128
    d = 128
    _, q2, planes2, dctx2, _ = _case(L, T, nb, N, d)
    runs = {}
    for key in (0, 1):
        att, lse, sc = _forward(L, key, q2, planes2.data_ptr(), planes2.data_ptr(), d * ldp, ldp, plan, T, nb, N, 0.1, d=d)
        runs[key] = (att, lse, sc)
        if lib.csn_attn_bwd_dq_no_planes_available(d, T):
            runs[key] += _dq(L, key, planes2.data_ptr(), planes2.data_ptr(), d * ldp, ldp, plan, T, nb, N, 0.1, att, lse, sc, dctx2, d=d)[:2]
    same(runs)
    assert _count(L) == n0, "a 64-query instance was launched"


def test_module_step_bit_for_bit(L):
    """The folded CrossShapeAt training step (N = 1236: a short last block): ``tuning.wg64`` on against off."""
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    L.check(L.lib().csn_set_math_mode(1))
    n_cls, T, N = 7, 500, 1236
    p, x, nb, lab = orc.conditioned_csa_case(np.random.default_rng(4004 + N), B, K, 1, n_cls, 4.0, 2.0, 1.0, n_points=N)
    runs = {}
    for on in (False, True):
        model = get_model("csa", n_cls, 1, K, block=T, n_blocks=None)
        model.load_state_dict(p, strict=False)
        model = model.cuda().train(True)
        calls = []
        L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
        n0 = _count(L)
        try:
            torch.manual_seed(9)
            with tuning.override(wg64=on):
                loss = orc.masked_ce_loss(model(x.cuda(), "train", nb.cuda()), lab.cuda())
                loss.backward()
        finally:
            L.set_call_hook(None)
        assert "csn_fold_weights_f32" in calls, "the step did not fold"
        assert calls.count("csn_block_attn_bwd_dq_f32") == 1
        assert L.lib().csn_dev_get(L.DEV_ATTN_WG64) == int(on)
        assert _count(L) - n0 == int(on)
        runs[on] = (loss.detach(), {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    assert torch.equal(_bits(runs[True][0]), _bits(runs[False][0])), "loss"
    assert len(runs[True][1]) == len(runs[False][1]) == 11
    for n, g in runs[True][1].items():
        assert torch.equal(_bits(g), _bits(runs[False][1][n])), n
