"""The mix backward folded into the LayerNorm-backward stream (tuning.fused_mix_bwd, csn_outproj_lnb_f32, wx_lnb.hip): the
reductions rowdot / rowsum come out of the launch that runs the mixed evaluations, which the mix's backward starts itself.

Shapes: C = d = 256, one head, B = 2, K = 2 (train plan: 6 mixed + 4 + 2 pooled evaluations) at
  N = 132 in one block   — four 32-point chunks and a 4-point tail chunk per evaluation, one chunk per stream;
  N = 2000 in 4 blocks   — 63 chunks per evaluation, an odd count: with two chunks per stream a run crosses from one
                            evaluation into the next and has to flush its partial sums in the middle.
Each with fc / attention dropout 0.1 and 0.  bf16x3 only (the fused kernel exists in that mode alone).

Every test that goes through the module runs twice: with folded projections (tuning.folded_projections — W_fv^T travels through
the link into the mix's LayerNorm backward) and with the unfolded chain (W_fc^T formed in the backward, the dK / dV launches);
the call hook says which form ran."""
import numpy as np
import pytest
import torch

from oracle import csa_oracle as orc

pytestmark = pytest.mark.gpu
B, K, H, C, N_CLS = 2, 2, 1, 256, 7
K1 = K + 1
SHAPES = {132: (132, 1), 2000: (500, 4)}                # n_points -> (block, n_blocks)
CASES = [(n, p) for n in SHAPES for p in (0.1, 0.0)]
IDS = [f"N{n}-p{p}" for n, p in CASES]
TOL = 2e-4                                              # of tests/test_gpu_module.py::test_fused_data_flow_equals_the_unfused_one


def _with_fold(cases, ids):
    """every case with folded projections (the default: the id the case always had) and as the unfolded chain"""
    return [pytest.param(*(c if isinstance(c, tuple) else (c,)), fold, id=i + ("" if fold else "-unfolded"))
            for c, i in zip(cases, ids) for fold in (True, False)]


@pytest.fixture(autouse=True)
def bf16x3():
    from csn_amd import _lib
    _lib.build()
    _lib.check(_lib.lib().csn_set_math_mode(1))
    yield
    _lib.lib().csn_set_math_mode(1)


@pytest.fixture(scope="module")
def data():
    """Per point count: parameters, inputs, labels (oracle.conditioned_csa_case) — made once, never modified."""
    out = {}
    for n in SHAPES:
        out[n] = orc.conditioned_csa_case(np.random.default_rng(700 + n), B, K, H, N_CLS, 4.0, 3.0, 1.0, n_points=n)
    return out


def _model(p, n, drop, train=True):
    from csn_amd.csa_models import get_model
    block, n_blocks = SHAPES[n]
    m = get_model("csa", N_CLS, H, K, block=block, n_blocks=n_blocks)
    m.load_state_dict(p, strict=False)
    m = m.cuda()
    m = m.train() if train else m.eval()
    m.attention.dropout.p = drop
    m.attention.attention.dropout.p = drop
    return m


class _Calls:
    """Names of the launching library calls made inside the block."""

    def __enter__(self):
        from csn_amd import _lib
        self.names = []
        _lib.set_call_hook(lambda name, phase: self.names.append(name) if phase == "begin" else None)
        return self

    def __exit__(self, *exc):
        from csn_amd import _lib
        _lib.set_call_hook(None)


def _train_step(m, x, nb, lab):
    """CrossShapeAt._csa_cm + logits + loss on the TRAIN plan ("csa_train": the pooled self evaluation is one of its own),
    whatever the dropout rates — at rate 0 the module itself would pick the eval plan, whose k = 0 evaluation is mixed AND
    pooled and therefore keeps the unfolded backward."""
    from csn_amd import functional as CF
    att = m.attention
    n = x.shape[2]
    geo = att.geometry(n_points=n)
    x_all = nb.squeeze(-1).reshape(B * K1, C, n).contiguous()
    E1, E2 = B * K1, B * K
    with CF.math_mode(att.math_mode):
        xhat, xmix, sums = att.evaluate(x_all, att.plan("csa_train", B, K1, x.device), geo, n_head_evals=E1, want_sums=True,
                                        link_mix=True)
        gamma, beta = att.norm.weight, att.norm.bias
        means = sums / n
        pooled = torch.cat((means[E1 + E2:].view(B, 1, C), means[E1:E1 + E2].view(B, K, C)), dim=1) * gamma + beta
        comp = m._compatibility(pooled)
        logits = m._logits(CF.csa_mix(xmix, comp, gamma, beta, B, K1))
    loss = orc.masked_ce_loss(logits, lab)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.item(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}


def _ran_form(names, fold):
    """the call names of a step say which form ran: folded projections, or the unfolded chain with its dK / dV launches"""
    assert ("csn_tile_planes_f32" in names) == ("csn_unfold_wgrads_f32" in names) == ("csn_fold_weights_f32" in names) == fold
    assert ("csn_block_attn_bwd_dkv_f32" in names) == (not fold)


def _run(data, n, drop, fused, fold):
    from csn_amd import tuning
    p, x, nb, lab = data[n]
    m = _model(p, n, drop)
    torch.manual_seed(11)                               # the dropout masks' seeds come from torch's CPU generator
    with tuning.override(folded_projections=fold), tuning.override(fused_mix_bwd=fused), _Calls() as calls:
        out = _train_step(m, x.cuda(), nb.cuda().contiguous(), lab.cuda())
    _ran_form(calls.names, fold)
    return out + (calls.names,)


@pytest.mark.parametrize("n,drop,fold", _with_fold(CASES, IDS))
def test_train_step_with_the_fold_equals_the_step_without(data, n, drop, fold):
    """Switch on against off on the same masks: the separate pass is gone, the forward is untouched, all 11 gradients agree
    within the tolerance the data-flow switches are held to; two runs with the switch on give the same bits."""
    l_on, s_on, g_on, c_on = _run(data, n, drop, True, fold)
    l_on2, s_on2, g_on2, _ = _run(data, n, drop, True, fold)
    l_off, s_off, g_off, c_off = _run(data, n, drop, False, fold)
    assert "csn_outproj_lnb_f32" in c_on and "csn_mix_bwd_f32" not in c_on and "csn_outproj_ln_bwd_f32" not in c_on
    assert "csn_mix_bwd_f32" in c_off and "csn_outproj_ln_bwd_f32" in c_off and "csn_outproj_lnb_f32" not in c_off
    assert torch.equal(l_on, l_off) and s_on == s_off
    assert set(g_on) == set(g_off) and len(g_on) == 11
    for k in g_on:
        assert torch.equal(g_on[k], g_on2[k]), k
        err, scale = (g_on[k] - g_off[k]).abs().max().item(), g_off[k].abs().max().item()
        print(f"N={n} p={drop} {k}: on-off {err:.3e} of {scale:.3e}")
        assert err <= TOL * scale + 1e-9, k


@pytest.mark.parametrize("n,fold", _with_fold(list(SHAPES), [f"N{n}" for n in SHAPES]))
def test_train_plan_without_dropout_holds_the_1e4_contract_against_float64(data, n, fold):
    """At rate 0 the train plan computes what the reference computes: logits, loss and the 11 gradients against the float64
    oracle, with the fold on."""
    p, x, nb, lab = data[n]
    block, n_blocks = SHAPES[n]
    logits, loss, grads, calls = _run(data, n, 0.0, True, fold)
    assert "csn_outproj_lnb_f32" in calls
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref = orc.forward_csa(x.double(), nb.double(), p64, H, block=block, n_blocks=n_blocks)
    ref_loss = orc.masked_ce_loss(ref, lab)
    ref_loss.backward()
    assert (logits.cpu().double() - ref.detach()).abs().max().item() < 1e-4
    assert abs(loss - ref_loss.item()) < 1e-5
    assert len(grads) == 11
    for k, g in grads.items():
        r = p64[k].grad
        err, scale = (g.cpu().double() - r).abs().max().item(), r.abs().max().item()
        print(f"N={n} {k}: {err / scale:.3e} relative")
        assert err <= 1e-4 * scale, k


@pytest.mark.parametrize("n,drop", CASES, ids=IDS)
def test_pieces_of_the_layernorm_backward_give_the_bits_of_the_one_call(n, drop):
    """The raw entry points on the train plan's geometry (12 evaluations, the first 6 mixed in groups of 3): evaluations
    [0, 6) with the reductions, [6, 12) with the row constants, then the W_fc gradient over all of dz — dz, dz_res, dCtx of
    every evaluation and dW_fc bit-equal to csn_outproj_ln_bwd_f32; rowdot / rowsum against float64 sums.
    Their bound: a sum here is at most 10 roundings deep (4 points by an fma chain, 8 lanes in 3 steps, at most 2 chunks of a
    stream in its cell — ceil(6 * 63 / 256) — and the fp32 result; the partials of the streams are added in fp64), so
    |error| <= 16 * 2^-24 * sum |terms| with room to spare."""
    from csn_amd import _lib, functional as CF
    L = _lib.lib()
    E, n_head, group = B * K1 + B * K + B, B * K1, K1
    gen = torch.Generator(device="cuda").manual_seed(n)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    xhat, att, dfeats = rnd(E, C, n), rnd(E, C, n), rnd(B, C, n)
    rstd = torch.rand(E, n, device="cuda", generator=gen) + 0.5
    scale, rows, w_t = rnd(n_head, C), rnd(E, C), rnd(C, C) / 16
    rows[:n_head] = 0                                   # the mixed evaluations carry no pooled-mean gradient
    seed, ptr, st = 12345, CF._ptr, CF._stream()
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    ws_n = L.csn_wgrad_workspace_floats(C, C, E, n)

    def whole():
        dz, dzr, dctx, dw, ws = new(E, C, n), new(E, C, n), new(E, C, n), new(C, C), torch.empty(ws_n, device="cuda")
        _lib.check(L.csn_outproj_ln_bwd_f32(ptr(dfeats), ptr(xhat), ptr(rstd), C * n, ptr(att), C * n, ptr(w_t), ptr(dz), ptr(dzr),
                                            ptr(dctx), ptr(dw), ptr(ws), ws_n, E, C, C, n, n, 0, drop, seed, 0, 0, ptr(rows), n_head,
                                            ptr(scale), group, st), "csn_outproj_ln_bwd_f32")
        return dz, dzr, dctx, dw

    def pieces():
        dz, dzr, dctx, dw, ws = new(E, C, n), new(E, C, n), new(E, C, n), new(C, C), torch.empty(ws_n, device="cuda")
        assert L.csn_outproj_lnb_workspace_floats(E, C, C, n, n) > 0
        red_n = L.csn_outproj_lnb_workspace_floats(n_head, C, C, n, n)
        red, rowdot, rowsum = new(red_n), new(n_head, C), new(n_head // group, C)
        _lib.check(L.csn_outproj_lnb_f32(ptr(dfeats), ptr(xhat), ptr(rstd), C * n, ptr(w_t), ptr(dz), ptr(dzr), ptr(dctx), 0, n_head,
                                         C, C, n, n, drop, seed, None, n_head, ptr(scale), group, ptr(rowdot), ptr(rowsum), ptr(red),
                                         red_n, st), "csn_outproj_lnb_f32")
        _lib.check(L.csn_outproj_lnb_f32(ptr(dfeats), ptr(xhat), ptr(rstd), C * n, ptr(w_t), ptr(dz), ptr(dzr), ptr(dctx), n_head,
                                         E - n_head, C, C, n, n, drop, seed, ptr(rows), n_head, ptr(scale), group, None, None, None, 0,
                                         st), "csn_outproj_lnb_f32")
        _lib.check(L.csn_project_wgrad_f32(ptr(dz), C * n, n, ptr(att), C * n, n, ptr(dw), C, C, E, n, 1.0, 0, ptr(ws), ws_n, st),
                   "csn_project_wgrad_f32")
        return dz, dzr, dctx, dw, rowdot, rowsum

    with CF.math_mode(1):
        one = whole()
        two = pieces()
        again = pieces()
    torch.cuda.synchronize()
    for name, a, b in zip(("dz", "dz_res", "dctx"), one, two):
        assert torch.isfinite(a).all(), name
        for e in range(E):
            assert torch.equal(a[e], b[e]), (name, e)
    assert torch.isfinite(one[3]).all() and torch.equal(one[3], two[3])
    assert torch.equal(two[4], again[4]) and torch.equal(two[5], again[5])
    g64, x64 = dfeats.double().repeat_interleave(group, dim=0), xhat[:n_head].double()
    bound = 16 * 2.0 ** -24
    err_dot = ((two[4].double() - (g64 * x64).sum(-1)).abs() / (g64 * x64).abs().sum(-1)).max().item()
    err_sum = ((two[5].double() - dfeats.double().sum(-1)).abs() / dfeats.double().abs().sum(-1)).max().item()
    print(f"N={n} p={drop}: rowdot {err_dot:.3e}, rowsum {err_sum:.3e} of sum |terms| (bound {bound:.3e})")
    assert err_dot <= bound and err_sum <= bound


def test_eval_mode_with_gradients_keeps_the_unfolded_backward(data):
    """Eval mode, plan "csa": the k = 0 evaluation is mixed and pooled, so the old path runs whatever the switch says — same
    calls, same bits.  ("unfolded" in the name: the mix backward is not folded into the LayerNorm backward; the projections fold
    or not as ``fold`` says, once each)"""
    for fold in (True, False):
        _eval_mode_with_gradients(data, fold)


def _eval_mode_with_gradients(data, fold):
    from csn_amd import tuning
    p, x, nb, lab = data[132]
    outs = []
    for fused in (True, False):
        m = _model(p, 132, 0.1, train=False)
        with tuning.override(folded_projections=fold), tuning.override(fused_mix_bwd=fused), _Calls() as calls:
            logits = m(x.cuda(), "test", nb.cuda().contiguous())
            orc.masked_ce_loss(logits, lab.cuda()).backward()
            torch.cuda.synchronize()
        _ran_form(calls.names, fold)
        assert "csn_mix_bwd_f32" in calls.names and "csn_outproj_lnb_f32" not in calls.names
        outs.append((logits.detach(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}))
    assert torch.equal(outs[0][0], outs[1][0]) and len(outs[0][1]) == 11
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("dense_too", [False, True], ids=["linked-only", "maps-also-dense"])
def test_functional_gradients_with_fixed_upstream_gradients(data, dense_too):
    """mha_evals + csa_mix with comp a leaf and the pooled sums weighted by constants: dfeats and the row constants are then
    the same numbers with the switch on and off, so everything that follows from dz and dCtx — the four weight gradients and
    the input gradient (dz_res) — must be the same BITS; d comp / d gamma / d beta agree to rounding.  dense_too: the caller
    also consumes the maps densely — the early launch is overwritten by the full one."""
    from csn_amd import functional as CF, tuning
    p, x, nb, _ = data[132]
    n = 132
    gen = torch.Generator(device="cuda").manual_seed(5)
    E = B * K1 + B * K + B
    w_feats, w_sums = torch.randn(B, C, n, device="cuda", generator=gen), torch.randn(E, C, device="cuda", generator=gen)
    w_sums[:B * K1] = 0
    w_maps = torch.randn(E, C, n, device="cuda", generator=gen)
    comp0 = torch.softmax(torch.randn(B, K1, device="cuda", generator=gen), dim=1)
    outs = []
    for fused in (True, False):
        m = _model(p, n, 0.1)
        att = m.attention
        x_all = nb.squeeze(-1).reshape(B * K1, C, n).contiguous().cuda().requires_grad_(True)
        comp = comp0.clone().requires_grad_(True)
        torch.manual_seed(17)
        with tuning.override(fused_mix_bwd=fused), _Calls() as calls, CF.math_mode(att.math_mode):
            xhat, xmix, sums = att.evaluate(x_all, att.plan("csa_train", B, K1, x_all.device), att.geometry(n_points=n),
                                            n_head_evals=B * K1, want_sums=True, link_mix=True)
            feats = CF.csa_mix(xmix, comp, att.norm.weight, att.norm.bias, B, K1)
            loss = (feats * w_feats).sum() + (sums * w_sums).sum()
            if dense_too:
                loss = loss + (xhat * w_maps).sum()
            loss.backward()
            torch.cuda.synchronize()
        assert ("csn_outproj_lnb_f32" in calls.names) == fused
        assert ("csn_outproj_ln_bwd_f32" in calls.names) == (dense_too or not fused)
        _ran_form(calls.names, False)                   # (input gradients wanted: the projections are never folded here)
        g = {k: q.grad.clone() for k, q in att.named_parameters() if q.grad is not None}
        g["x_all"], g["comp"] = x_all.grad.clone(), comp.grad.clone()
        outs.append(g)
    on, off = outs
    assert set(on) == set(off)
    for k in ("w_qs.weight", "w_ks.weight", "w_vs.weight", "fc.weight", "x_all"):
        assert torch.equal(on[k], off[k]), k
    for k in ("comp", "norm.weight", "norm.bias"):
        assert (on[k] - off[k]).abs().max().item() <= TOL * off[k].abs().max().item() + 1e-9, k
