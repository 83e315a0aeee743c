"""Folded projections (include/csn_hip.h (1b), tuning.folded_projections): W_k folded into W_q, W_v into W_fc, the attention on the
tile planes of x itself.

1. csn_tile_planes_f32 bit for bit against a numpy restatement of csn_mode::split4, zero padding and unwritten tiles included; the
   same planes read by the forward entry point and written by csn_project_f32(out_split = 2) with an identity weight.
2. the dQ instance without planes (probs_tiles = 3): dQ and delta bit-equal to probs_tiles = 2, scores untouched, dscores = NULL.
3. csn_fold_weights_f32 / csn_unfold_wgrads_f32 against float64 numpy within the bound of a 256-long fp32 dot product, the same
   bits in math modes 1 and 2.
4. the module step folded and unfolded, both against the float64 oracle with the masks of tests/dropout_ref.py, at the project's
   contract (1e-4 of the tensor's max-abs; the compatibility head with the noise term of test_gpu_module._grad_check).
5. declined cases (input gradients, two heads) keep the bits of the switched-off step.
6. eval-mode logits with and without autograd are the same bits."""
import numpy as np
import pytest
import torch

from oracle import csa_oracle as orc
from tests import attn_edge_ref as ar
from tests import dropout_ref as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_thread_score_layout(0)
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)
    L.set_call_hook(None)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the planes kernel ------------------------------------------------------------------------------------------------
def _bf16_rne(x):
    """fp32 array -> the bf16 bits (uint16) of round-to-nearest-even, as csn_mode::to16<false> (finite inputs)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


SENTINEL = 0x7FC1                  # a bf16 NaN no kernel writes: what the buffer holds where nothing was written


def _planes_ref(x, T, ldp):
    """numpy restatement: per row and block of T points 16 tiles of [hi 32 | lo 32], hi = bf16(x), lo = bf16(x - hi); the padding
    keys of every block's last tile zeros; tiles beyond a (short) block's last key untouched"""
    S, C, NP = x.shape
    nb = (NP + T - 1) // T
    out = np.full((S, C, ldp), SENTINEL, dtype=np.uint16)
    hi = _bf16_rne(x)
    lo = _bf16_rne(x - _bf16_val(hi))
    for b in range(nb):
        t_blk = min(T, NP - b * T)
        for t in range((t_blk + 31) // 32):
            n = min(32, t_blk - 32 * t)
            base = b * 1024 + t * 64
            out[:, :, base:base + 64] = 0
            src = slice(b * T + 32 * t, b * T + 32 * t + n)
            out[:, :, base:base + n] = hi[:, :, src]
            out[:, :, base + 32:base + 32 + n] = lo[:, :, src]
    return out


@pytest.mark.parametrize("NP,T", [(1500, 500), (1236, 500), (108, 36)], ids=["3x500", "short-last-block", "two-tiles-4-keys"])
def test_tile_planes_bit_for_bit(L, NP, T):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    rng = np.random.default_rng(NP + T)
    S, C = 3, 256
    nb = (NP + T - 1) // T
    ldp = nb * 1024
    x = (rng.standard_normal((S, C, NP)) * np.exp(rng.uniform(-2, 2, (S, C, 1)))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    guard = 64
    buf = torch.full((S * C * ldp + 2 * guard,), SENTINEL, dtype=torch.int16, device="cuda")
    out = buf[guard:guard + S * C * ldp]
    L.check(lib.csn_tile_planes_f32(xd.data_ptr(), C * NP, NP, out.data_ptr(), C * ldp, ldp, S, C, NP, T, _stream()), "planes")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16).reshape(S, C, ldp)
    want = _planes_ref(x, T, ldp)
    assert np.array_equal(got, want)
    g = buf.cpu().numpy().view(np.uint16)
    assert (g[:guard] == SENTINEL).all() and (g[-guard:] == SENTINEL).all(), "wrote outside the planes"

    # the same layout as the projection's: identity weight, out_split = 2.  The projection forms hi + lo in fp32 and splits the
    # sum again, which moves lo by one bf16 ulp where lo was rounded up to half an ulp of hi — so: the same elements written,
    # the same values to 2^-16 of |x|, and nearly all of them the same bits
    eye = torch.eye(C, device="cuda")
    pbuf = torch.full((S, C, ldp), SENTINEL, dtype=torch.int16, device="cuda")
    L.check(lib.csn_project_f32(xd.data_ptr(), C * NP, NP, eye.data_ptr(), C, C, pbuf.data_ptr(), C * ldp, ldp, S, NP, 0, 1.0, 2, T,
                                _stream()), "identity projection")
    torch.cuda.synchronize()
    proj = pbuf.cpu().numpy().view(np.uint16)
    assert np.array_equal(proj == SENTINEL, got == SENTINEL), "the projection writes other elements"
    w = got != SENTINEL
    val = lambda p: _bf16_val(np.where(w, p, 0).reshape(S, C, nb, 16, 2, 32)).astype(np.float64).sum(axis=4)
    scale = np.abs(x).max(axis=2).reshape(S, C, 1, 1, 1)
    assert (np.abs(val(proj) - val(got)) <= 2.0 ** -16 * scale).all()
    assert (proj[w] == got[w]).mean() > 0.99

    # ... and as the forward entry point reads them: K = V = the planes of x, against the projection's planes
    E, H, d, Tp = S, 1, C, (T + 31) // 32 * 32
    NPP = nb * T
    q = torch.from_numpy((rng.standard_normal((S, C, NP)) / 16).astype(np.float32)).cuda()
    idx = torch.arange(E, dtype=torch.int32, device="cuda")
    res = []
    for planes in (out, pbuf):
        ctx = torch.zeros((E, C, NP), device="cuda")
        lse = torch.zeros((E, H, NPP), device="cuda")
        L.check(lib.csn_block_attn_fwd_f32(q.data_ptr(), planes.data_ptr(), planes.data_ptr(), C * NP, C * ldp, idx.data_ptr(),
                                           idx.data_ptr(), NP, ctx.data_ptr(), C * NP, None, lse.data_ptr(), E, H, d, T, nb, Tp, 8.0,
                                           0.0, 0, 1, ldp, _stream()), "forward")
        res.append((ctx, lse))
    torch.cuda.synchronize()
    (c0, l0), (c1, l1) = res
    assert torch.isfinite(c0).all() and torch.isfinite(l0[..., :NP]).all()
    assert (c0 - c1).abs().max().item() <= 1e-5 * c1.abs().max().item()
    assert (l0[..., :NP] - l1[..., :NP]).abs().max().item() <= 1e-5
    # float64: softmax(q^T x) x^T over each block
    xq, x64 = q.double().cpu(), torch.from_numpy(x).double()
    for b in range(nb):
        sl = slice(b * T, min(NP, (b + 1) * T))
        pr = torch.softmax(xq[:, :, sl].transpose(1, 2) @ x64[:, :, sl], dim=-1)
        ref = (pr @ x64[:, :, sl].transpose(1, 2)).transpose(1, 2)
        assert (c0[:, :, sl].cpu().double() - ref).abs().max().item() <= ar.BOUNDS[1][0] * ref.abs().max().item()


def test_tile_planes_refuses_what_it_cannot_lay_out(L):
    lib = L.lib()
    z = torch.zeros(4096, device="cuda")
    p = z.data_ptr()
    assert lib.csn_tile_planes_f32(p, 0, 1000, p, 0, 1024, 1, 1, 1000, 500, _stream()) == -1      # two blocks, one block's pitch
    assert lib.csn_tile_planes_f32(p, 0, 1000, p, 0, 2048, 1, 1, 1000, 516, _stream()) == -1      # block > 512
    assert lib.csn_tile_planes_f32(p, 0, 1002, p, 0, 3072, 1, 1, 1002, 500, _stream()) == -2      # points % 4
    assert lib.csn_tile_planes_f32(None, 0, 1000, p, 0, 2048, 1, 1, 1000, 500, _stream()) == -1


# ---- 2. the dQ instance without planes -------------------------------------------------------------------------------------
Q_IDX, KV_IDX = (0, 0, 0, 1), (0, 1, 2, 1)              # one query group of three evaluations, one of one


def _dq_cases():
    out = []
    for T, nb in ((500, 2), (36, 3), (128, 1)):
        for p in (0.0, 0.1):
            for layout in ((0, 1) if ar.grouping(1, 256, T) & 16 else (0,)):
                out.append((T, nb, p, layout))
    return out


@pytest.mark.parametrize("T,nb,p,layout", _dq_cases(), ids=lambda v: str(v))
def test_dq_without_planes(L, T, nb, p, layout):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    d = D = 256
    H, S, E = 1, 3, 4
    assert lib.csn_attn_bwd_dq_no_planes_available(d, T) and not lib.csn_attn_bwd_dq_no_planes_available(128, T)
    L.check(lib.csn_set_thread_score_layout(layout))
    rng = np.random.default_rng(1000 * T + nb)
    N, Tp, seed = T * nb, (T + 31) // 32 * 32, ar.HIGH_SEED + T
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    q, k, v, dctx = rnd(S, D, N) / 4, rnd(S, D, N) / 4, rnd(S, D, N), rnd(E, D, N)
    ldp = nb * ar.BLOCK_PITCH * 2
    kv = ar.pack_tile_planes(torch.cat((k, v), 1), T, nb, 2, "bf16", None).cuda().contiguous()
    k_ptr, v_ptr, kvs = kv.data_ptr(), kv.data_ptr() + 2 * D * ldp, 2 * D * ldp
    qd, dd = q.cuda(), dctx.cuda()
    qi = torch.tensor(Q_IDX, dtype=torch.int32, device="cuda")
    ki = torch.tensor(KV_IDX, dtype=torch.int32, device="cuda")
    ctx = torch.zeros((E, D, N), device="cuda")
    lse = torch.zeros((E, H, N), device="cuda")
    sc = torch.full((E, H, nb, T, Tp), float("nan"), device="cuda")
    L.check(lib.csn_block_attn_fwd_f32(qd.data_ptr(), k_ptr, v_ptr, D * N, kvs, qi.data_ptr(), ki.data_ptr(), N, ctx.data_ptr(), D * N,
                                       sc.data_ptr(), lse.data_ptr(), E, H, d, T, nb, Tp, 8.0, p, seed, 1, ldp, _stream()), "forward")
    from csn_amd.functional import EvalPlan
    plan = EvalPlan(np.array(Q_IDX), np.array(KV_IDX), S, "cuda")
    assert plan.n_q_groups == 2

    def dq_call(probs_tiles):
        scb = sc.clone()
        ds = torch.full_like(sc, float("nan")) if probs_tiles != 3 else None
        delta = torch.full((E, H, N), float("nan"), device="cuda")
        dq = torch.full((S, D, N), float("nan"), device="cuda")
        L.check(lib.csn_block_attn_bwd_dq_f32(dd.data_ptr(), ctx.data_ptr(), D * N, k_ptr, v_ptr, kvs, ki.data_ptr(), N, scb.data_ptr(),
                                              ds.data_ptr() if ds is not None else None, lse.data_ptr(), delta.data_ptr(),
                                              dq.data_ptr(), D * N, qi.data_ptr(), 0, plan.q_group_items.data_ptr(), E, H, d, T, nb,
                                              Tp, p, seed, 0, 0, 1, ldp, probs_tiles, plan.q_group_off.data_ptr(), plan.n_q_groups,
                                              _stream()), f"dq, probs_tiles = {probs_tiles}")
        torch.cuda.synchronize()
        return scb, delta, dq

    sc2, delta2, dq2 = dq_call(2)
    sc3, delta3, dq3 = dq_call(3)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(sc3), bits(sc)) and torch.equal(bits(sc2), bits(sc)), "the scores were touched"
    assert torch.equal(bits(delta3), bits(delta2)), "delta differs"
    assert torch.equal(bits(dq3), bits(dq2)), "dQ differs"
    assert torch.isfinite(dq3[:2]).all() and torch.isnan(dq3[2]).all()        # slots 0 and 1 written, slot 2 (no queries) untouched


def test_dq_without_planes_is_refused_elsewhere(L):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    z = torch.zeros(64, device="cuda")
    p = z.data_ptr()
    call = lambda d, pt: lib.csn_block_attn_bwd_dq_f32(p, p, 0, p, p, 0, None, 36, p, None, p, p, p, 0, None, 0, None, 1, 1, d, 36, 1, 64,
                                                       0.0, 0, 0, 0, 1, 1024, pt, None, 0, _stream())
    assert call(128, 3) == -1 and call(256, 4) == -1
    L.check(lib.csn_set_math_mode(2))
    assert not lib.csn_attn_bwd_dq_no_planes_available(256, 500) and call(256, 3) == -1


# ---- 3. fold and unfold --------------------------------------------------------------------------------------------------------
def test_fold_and_unfold_are_exact_fp32_in_every_mode(L):
    lib = L.lib()
    rng = np.random.default_rng(31)
    D = C = 256
    t = 16.0
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    w = {n: u(D, C) / 16 for n in ("q", "k", "v")}
    w["fc"] = u(C, D) / 4
    dm, dwfv = u(C, C), u(C, C)
    dev = {n: torch.from_numpy(a).cuda() for n, a in w.items()}
    dmd, dwfvd = torch.from_numpy(dm).cuda(), torch.from_numpy(dwfv).cuda()
    f8 = {n: a.astype(np.float64) for n, a in w.items()}
    ab = {n: np.abs(a) for n, a in f8.items()}
    eps = 256 * 2.0 ** -24
    # (want, bound = eps * sum |a| |b|): the products, and the division by t as one more rounding of the result
    want = {
        "m": (f8["k"].T @ f8["q"] / t, eps * (ab["k"].T @ ab["q"]) / t),
        "w_fv": (f8["fc"] @ f8["v"], eps * (ab["fc"] @ ab["v"])),
        "w_fv_t": ((f8["fc"] @ f8["v"]).T, eps * (ab["fc"] @ ab["v"]).T),
        "dw_q": (f8["k"] @ dm.astype(np.float64) / t, eps * (ab["k"] @ np.abs(dm)) / t),
        "dw_k": (f8["q"] @ dm.astype(np.float64).T / t, eps * (ab["q"] @ np.abs(dm).T) / t),
        "dw_fc": (dwfv.astype(np.float64) @ f8["v"].T, eps * (np.abs(dwfv) @ ab["v"].T)),
        "dw_v": (f8["fc"].T @ dwfv.astype(np.float64), eps * (ab["fc"].T @ np.abs(dwfv))),
    }
    assert lib.csn_fold_workspace_floats(D, C) == 2 * D * C
    runs = {}
    for mode in (1, 2):
        L.check(lib.csn_set_thread_math_mode(mode))
        out = {n: torch.full((256, 256), float("nan"), device="cuda") for n in want}
        ws = torch.empty(2 * D * C, device="cuda")
        L.check(lib.csn_fold_weights_f32(dev["q"].data_ptr(), dev["k"].data_ptr(), dev["v"].data_ptr(), dev["fc"].data_ptr(), D, C, t,
                                         out["m"].data_ptr(), out["w_fv"].data_ptr(), out["w_fv_t"].data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream()), "fold")
        L.check(lib.csn_unfold_wgrads_f32(dmd.data_ptr(), dwfvd.data_ptr(), dev["q"].data_ptr(), dev["k"].data_ptr(), dev["v"].data_ptr(),
                                          dev["fc"].data_ptr(), D, C, t, out["dw_q"].data_ptr(), out["dw_k"].data_ptr(),
                                          out["dw_v"].data_ptr(), out["dw_fc"].data_ptr(), ws.data_ptr(), D * C, _stream()), "unfold")
        torch.cuda.synchronize()
        runs[mode] = {n: o.cpu().numpy() for n, o in out.items()}
    L.check(lib.csn_set_thread_math_mode(-1))
    for n, (ref, bound) in want.items():
        err = np.abs(runs[1][n].astype(np.float64) - ref)
        print(f"[fold] {n}: max error {err.max():.3e}, tightest margin {(bound - err).min():.3e}")
        assert (err <= bound).all(), n
        assert np.array_equal(runs[1][n].view(np.uint32), runs[2][n].view(np.uint32)), f"{n} inherits the math mode"
    ws = torch.empty(16, device="cuda")
    assert lib.csn_fold_weights_f32(dev["q"].data_ptr(), dev["k"].data_ptr(), dev["v"].data_ptr(), dev["fc"].data_ptr(), D, C, t,
                                    dev["q"].data_ptr(), dev["q"].data_ptr(), dev["q"].data_ptr(), ws.data_ptr(), 16, _stream()) == -6


# ---- 4. the module step, folded against unfolded, both against float64 ------------------------------------------------------
def _masked_oracle(p, x, nb, lab, dtype, T, n_blocks, B, K, seeds, p_drop, masks=None, evals_of=None):
    """orc.forward_csa in `dtype` with an mha that applies the step's own masks (tests/dropout_ref.py) — evaluation numbering of
    MultiHeadAttention.plan("csa_train") / ("csa"); seeds None: eval mode.
    masks = (attention mask [e][blk][query][key], fc mask [e][c][n]) together with evals_of(call) -> the B evaluations of the
    oracle's call-th mha call (pooled self, neighbour self k = 1..K, mixed self, mixed cross k = 1..K): a step that numbers its
    evaluations otherwise or draws several seed pairs (the two-phase step, tests/test_gpu_folded_plans.py)"""
    K1 = K + 1
    E1, E2 = B * K1, B * K
    N = x.shape[2]
    C = x.shape[1]
    Tp = (T + 31) // 32 * 32
    train = seeds is not None or masks is not None
    E = E1 + E2 + (B if train else 0)
    if masks is not None:
        am, fm = masks
    elif train:
        am = torch.from_numpy(dr.attention_mask(E, 1, n_blocks, T, Tp, seeds[0], p_drop))[:, 0].transpose(-1, -2)   # [e][blk][query][key]
        fm = torch.from_numpy(dr.fc_mask(E, C, N, seeds[1], p_drop))                                                  # [e][c][n]
    q = {k_: v_.to(dtype).clone().requires_grad_(True) for k_, v_ in p.items()}
    calls = []

    def plan_evals_of(call):
        # csa_feats: pooled self, neighbour self k = 1..K, mixed self, mixed cross k = 1..K
        if call == 0:
            return [E1 + E2 + b if train else b * K1 for b in range(B)]
        if call <= K:
            return [E1 + b * K + call - 1 for b in range(B)]
        k_ = call - K - 1
        return [b * K1 + k_ for b in range(B)]

    evals_of = evals_of or plan_evals_of

    def mha(xq, xk, xv, prm, n_head, **kw):
        ev = evals_of(len(calls))
        calls.append(ev)
        a = xq.squeeze(-1).permute(0, 2, 1)
        b_ = xk.squeeze(-1).permute(0, 2, 1)
        wq, wk, wv, wfc = (prm[f"attention.{n}.weight"] for n in ("w_qs", "w_ks", "w_vs", "fc"))
        outs = []
        for blk in range(n_blocks):
            sl = slice(blk * T, min(N, (blk + 1) * T))
            t_b = sl.stop - sl.start
            Q = a[:, sl] @ wq.t() / (wq.shape[0] ** 0.5)
            Kk, V = b_[:, sl] @ wk.t(), b_[:, sl] @ wv.t()
            pr = torch.softmax(Q @ Kk.transpose(1, 2), dim=-1)
            if train:
                pr = pr * am[ev, blk, :t_b, :t_b].to(dtype) / (1.0 - p_drop)
            z = (pr @ V) @ wfc.t()
            if train:
                z = z * fm[ev][:, :, sl].permute(0, 2, 1).to(dtype) / (1.0 - p_drop)
            z = z + a[:, sl]
            outs.append(torch.nn.functional.layer_norm(z, (C,), prm["attention.norm.weight"], prm["attention.norm.bias"], 1e-6))
        return torch.cat(outs, dim=1)

    logits = orc.forward_csa(x.to(dtype), nb.to(dtype), q, 1, mha=mha)
    loss = orc.masked_ce_loss(logits, lab)
    loss.backward()
    assert len(calls) == 2 * K + 2
    return logits.detach(), loss.item(), {k_: v_.grad for k_, v_ in q.items()}


def _module_step(L, p, x, nb, lab, n_cls, K, geo, train, fold, seed=9):
    from csn_amd import functional as CF, tuning
    from csn_amd.csa_models import get_model
    model = get_model("csa", n_cls, 1, K, **geo)
    model.load_state_dict(p, strict=False)
    model = model.cuda().train(train)
    calls, seeds = [], []
    draw = CF.draw_seeds

    def recording(n):
        s = draw(n)
        seeds.append(s)
        return s

    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    CF.draw_seeds = recording
    try:
        torch.manual_seed(seed)
        with tuning.override(folded_projections=fold):
            logits = model(x.cuda(), "train" if train else "test", nb.cuda())
            loss = orc.masked_ce_loss(logits, lab.cuda())
            loss.backward()
    finally:
        CF.draw_seeds = draw
        L.set_call_hook(None)
    grads = {n: q.grad.detach().cpu() for n, q in model.named_parameters() if q.grad is not None}
    return logits.detach().cpu(), loss.item(), grads, calls, (seeds[0] if seeds else None)


_step_refs = {}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("N", [1500, 1236], ids=["3x500", "short-last-block"])
def test_module_step_folded_and_unfolded_against_float64(L, N, train):
    """Both forms are held to the float64 oracle at the project's contract: logits and each of the 11 gradients within 1e-4 of
    the reference tensor's max-abs; the four compatibility-head tensors with _grad_check's noise term (10 x the deviation of the
    same oracle run in fp32 from the float64 one).  Nothing tighter is asserted between the two forms."""
    L.check(L.lib().csn_set_math_mode(1))
    B, K, n_cls, T, n_blocks = 2, 2, 7, 500, 3
    geo = dict(block=T, n_blocks=n_blocks if N == T * n_blocks else None)      # (None: every point, the last block short)
    p, x, nb, lab = orc.conditioned_csa_case(np.random.default_rng(4004 + N), B, K, 1, n_cls, 4.0, 2.0, 1.0, n_points=N)
    runs = {fold: _module_step(L, p, x, nb, lab, n_cls, K, geo, train, fold) for fold in (True, False)}
    assert "csn_tile_planes_f32" in runs[True][3] and "csn_fold_weights_f32" in runs[True][3] and "csn_unfold_wgrads_f32" in runs[True][3]
    assert "csn_block_attn_bwd_dkv_f32" not in runs[True][3] and "csn_block_attn_bwd_dv_scores_f32" not in runs[True][3]
    assert "csn_tile_planes_f32" not in runs[False][3] and "csn_block_attn_bwd_dkv_f32" in runs[False][3]
    seeds = runs[True][4]
    assert seeds == runs[False][4] and (seeds is not None) == train
    ref64 = _masked_oracle(p, x, nb, lab, torch.float64, T, n_blocks, B, K, seeds, 0.1)
    ref32 = _masked_oracle(p, x, nb, lab, torch.float32, T, n_blocks, B, K, seeds, 0.1)
    r_logits, r_loss, r_grads = ref64
    worst = {}
    for fold in (True, False):
        logits, loss, grads = runs[fold][:3]
        assert len(grads) == 11
        e_log = (logits.double() - r_logits).abs().max().item() / r_logits.abs().max().item()
        print(f"[folded-step] N={N} train={train} fold={fold}: logits {e_log:.2e} loss {abs(loss - r_loss):.2e}")
        worst[fold] = {"logits": (e_log, 1e-4)}
        for n, g in grads.items():
            r = r_grads[n].double()
            scale = r.abs().max().item()
            noise = (ref32[2][n].double() - r).abs().max().item() if n.startswith("compatibility") else 0.0
            err = (g.double() - r).abs().max().item()
            print(f"[folded-step]   {n}: {err / scale:.2e} of max-abs (allowed {1e-4 + 10.0 * noise / scale:.2e})")
            worst[fold][n] = (err, 1e-4 * scale + 10.0 * noise)
        worst[fold]["loss"] = (abs(loss - r_loss), 1e-5)
    for fold in (True, False):
        for n, (err, lim) in worst[fold].items():
            assert err <= lim, (("folded" if fold else "unfolded"), n, err, lim)


def test_masks_are_identical_where_the_two_forms_coincide(L):
    """W_k = W_v = I: M = W_q / t and W_fv = W_fc, the two forms run the same products on the same numbers (K = V = x to fp32
    rounding), so with the same masks their train-mode losses agree to the loss contract (1e-5) — another mask would move the
    loss by orders of magnitude more (the same step under another seed, below)."""
    L.check(L.lib().csn_set_math_mode(1))
    B, K, n_cls, T, n_blocks, N = 2, 2, 7, 500, 3, 1500
    p, x, nb, lab = orc.conditioned_csa_case(np.random.default_rng(5150), B, K, 1, n_cls, 4.0, 2.0, 0.25, n_points=N)
    p["attention.w_ks.weight"] = torch.eye(256)
    p["attention.w_vs.weight"] = torch.eye(256)
    geo = dict(block=T, n_blocks=n_blocks)
    lf = _module_step(L, p, x, nb, lab, n_cls, K, geo, True, True)
    lu = _module_step(L, p, x, nb, lab, n_cls, K, geo, True, False)
    other = _module_step(L, p, x, nb, lab, n_cls, K, geo, True, True, seed=10)
    print(f"[folded-masks] loss folded {lf[1]:.8f} unfolded {lu[1]:.8f} other seed {other[1]:.8f}")
    assert "csn_tile_planes_f32" in lf[3] and lf[4] == lu[4] and other[4] != lf[4]
    assert abs(lf[1] - lu[1]) <= 1e-5
    assert abs(other[1] - lf[1]) > 1e-4, "the masks do not move this loss: the check above shows nothing"
    assert (lf[0] - lu[0]).abs().max().item() <= 1e-4 * lu[0].abs().max().item()


# ---- 5. declined cases keep their bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["input-gradients", "two-heads"])
def test_declined_cases_keep_their_bits(L, case):
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    L.check(L.lib().csn_set_math_mode(1))
    rng = np.random.default_rng(66)
    B, K, n_cls, N = 2, 1, 7, 200
    H = 2 if case == "two-heads" else 1
    torch.manual_seed(5)
    model = get_model("csa", n_cls, H, K, block=100, n_blocks=2).cuda().train(True)
    nbf = torch.from_numpy(rng.standard_normal((B, K + 1, 256, N, 1)).astype(np.float32))
    x = nbf[:, 0].contiguous()
    lab = torch.from_numpy(rng.integers(0, n_cls, size=(B, N))).cuda()
    outs = {}
    for fold in (True, False):
        for prm in model.parameters():
            prm.grad = None
        calls = []
        L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
        xd = x.cuda().requires_grad_(case == "input-gradients")
        nd = nbf.cuda()
        torch.manual_seed(9)
        with tuning.override(folded_projections=fold):
            logits = model(xd, "train", nd)
            orc.masked_ce_loss(logits, lab).backward()
        L.set_call_hook(None)
        assert "csn_tile_planes_f32" not in calls and "csn_fold_weights_f32" not in calls
        outs[fold] = [logits.detach()] + [q.grad.clone() for q in model.parameters() if q.grad is not None] + \
                     ([xd.grad.clone()] if xd.grad is not None else [])
    assert len(outs[True]) == len(outs[False]) == 12 + (case == "input-gradients")
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)


# ---- 6. the decision does not look at the grad mode -------------------------------------------------------------------------
def test_no_grad_logits_equal_grad_enabled_logits(L):
    from csn_amd.csa_models import get_model
    L.check(L.lib().csn_set_math_mode(1))
    rng = np.random.default_rng(67)
    B, K, n_cls, N = 2, 2, 7, 1000
    torch.manual_seed(5)
    model = get_model("csa", n_cls, 1, K, block=500, n_blocks=2).cuda().eval()
    nbf = torch.from_numpy(rng.standard_normal((B, K + 1, 256, N, 1)).astype(np.float32)).cuda()
    x = nbf[:, 0].contiguous()
    calls = []
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    with torch.no_grad():
        l0 = model(x, "test", nbf)
    n0 = calls.count("csn_tile_planes_f32")
    l1 = model(x, "test", nbf)
    L.set_call_hook(None)
    assert n0 == 1 and calls.count("csn_tile_planes_f32") == 2, "both forwards fold"
    assert l1.requires_grad and not l0.requires_grad
    assert torch.equal(l0, l1.detach())
