"""The float64 restatements of tests/tail_ref.py without a GPU: every hand-written backward against torch autograd of the forward
beside it (1e-12 of the tensor's maximum), the compatibility head's closed-form key rows against the reference's transpose /
reshape / view bookkeeping, and — on the restatements alone — what the cases of tests/test_gpu_tail.py rely on."""
import pytest
import torch
import torch.nn.functional as F

from tests import tail_ref as R

TOL = 1e-12


def _rel(got, want):
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("B,K1,C,NP", [(3, 8, 3, 4), (1, 2, 3, 1028), (3, 5, 1, 1028)])
def test_mix_backward_equals_autograd(B, K1, C, NP):
    t = R.mix_inputs(B, K1, C, NP)
    x, comp, gamma, beta = (t[n].double().requires_grad_() for n in ("xhat", "comp", "gamma", "beta"))
    feats, scale = R.mix_fwd(x, comp, gamma, beta)
    plain = (comp[:, :, None, None] * (x * gamma[None, None, :, None] + beta[None, None, :, None])).sum(dim=1)
    assert _rel(feats.detach(), plain.detach()) < TOL
    assert bool((scale >= feats.abs() * (1 - 1e-12)).all())
    feats.backward(t["dfeats"].double())
    dxhat, rowdot, rowsum, dot_abs, sum_abs = R.mix_bwd(t["dfeats"], t["xhat"], t["comp"], t["gamma"])
    assert _rel(dxhat, x.grad) < TOL
    assert bool((dot_abs >= rowdot.abs()).all()) and bool((sum_abs >= rowsum.abs()).all())
    (dcomp, a_c), (dgamma, a_g), (dbeta, a_b) = R.mix_param_grads(rowdot, rowsum, t["comp"], t["gamma"], t["beta"])
    # relative to the sum of |terms|: d comp is a difference of large numbers, its own maximum is not the scale of its rounding
    assert ((dcomp - comp.grad).abs() / a_c).max().item() < TOL
    assert ((dgamma - gamma.grad).abs() / a_g).max().item() < TOL
    assert ((dbeta - beta.grad).abs() / a_b).max().item() < TOL
    assert bool((a_c >= dcomp.abs()).all()) and bool((a_g >= dgamma.abs()).all()) and bool((a_b >= dbeta.abs()).all())


def _compat_autograd(t, ref_layout, forward):
    a = {n: t[n].double().clone().requires_grad_() for n in ("pooled", "wq", "bq", "wk", "bk")}
    comp = forward(a["pooled"], a["wq"], a["bq"], a["wk"], a["bk"], ref_layout)
    comp.backward(t["dcomp"].double())
    return comp.detach(), {n: v.grad for n, v in a.items()}


def _library_forward(pooled, wq, bq, wk, bk, ref_layout):
    """the head as the model writes it: nn.Linear, F.normalize, einsum, softmax"""
    u_q = F.normalize(F.linear(pooled[:, 0], wq, bq), dim=-1)
    u_k = F.normalize(F.linear(R.compat_keys(pooled, ref_layout), wk, bk), dim=-1)
    return F.softmax(torch.einsum("bc,bkc->bk", u_q, u_k), dim=-1)


@pytest.mark.parametrize("B,K1,C,ref_layout,beyond", R.COMPAT_CASES)
def test_compat_backward_equals_autograd(B, K1, C, ref_layout, beyond):
    t = R.compat_inputs(B, K1, C)
    comp, grads = R.compat(t["pooled"], t["wq"], t["bq"], t["wk"], t["bk"], ref_layout, t["dcomp"])
    for forward in (R.compat_fwd, _library_forward):
        c_ag, g_ag = _compat_autograd(t, ref_layout, forward)
        assert (comp - c_ag).abs().max().item() < TOL
        for n in grads:
            if K1 == 1:
                assert g_ag[n].abs().max().item() < 1e-15 and grads[n].abs().max().item() < 1e-15, n   # comp == 1: nothing to learn
            elif C == 1:                                                             # exactly zero but for a cancellation's rounding
                tol = R.compat_scalar_tol(t["pooled"], t["wq"], t["bq"], t["wk"], t["bk"], ref_layout, t["dcomp"])
                assert tol < 1e-6 and g_ag[n].abs().max().item() <= tol and grads[n].abs().max().item() <= tol, n
            else:
                assert _rel(grads[n], g_ag[n]) < TOL, n
    assert (B * K1 * C > C * C) == beyond
    if K1 == 1:
        assert bool((comp == 1).all())


@pytest.mark.parametrize("B,K1,C,ref_layout,zero_row", R.COMPAT_DEGENERATE)
def test_compat_degenerate_row_is_finite_and_equals_autograd(B, K1, C, ref_layout, zero_row):
    """A projected key of norm zero: F.normalize divides by the clamp, a constant, so the gradient there is du / 1e-12 — finite,
    about 1e11 to 1e12 — and everything else keeps its usual size."""
    t = R.compat_inputs(B, K1, C, zero_row=zero_row)
    comp, grads = R.compat(t["pooled"], t["wq"], t["bq"], t["wk"], t["bk"], ref_layout, t["dcomp"])
    keys = R.compat_keys(t["pooled"].double(), ref_layout) @ t["wk"].double().t() + t["bk"].double()
    assert int((keys.abs().amax(dim=-1) == 0).sum()) == 1                            # exactly one key row, exactly zero
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    b0, k0 = zero_row
    big = grads["pooled"][b0, k0].abs().max().item()
    assert 1e10 < big < 1e13 and 1e10 < grads["bk"].abs().max().item() < 1e13
    rest = grads["pooled"].clone()
    rest[b0, k0] = 0
    assert rest.abs().max().item() < 1e3 and all(grads[n].abs().max().item() < 1e3 for n in ("wq", "bq", "wk"))
    for forward in (R.compat_fwd, _library_forward):
        c_ag, g_ag = _compat_autograd(t, ref_layout, forward)
        assert (comp - c_ag).abs().max().item() < TOL
        assert _rel(grads["pooled"][b0, k0], g_ag["pooled"][b0, k0]) < TOL
        rest_ag = g_ag["pooled"].clone()
        rest_ag[b0, k0] = 0
        assert _rel(rest, rest_ag) < TOL
        for n in ("wq", "bq", "wk", "bk"):
            assert _rel(grads[n], g_ag[n]) < TOL, n


def _key_src_row(b, k, B, K1):
    """compat.hip's closed form: key row (b, k) of the head -> row of the (B, K1, C) descriptor tensor"""
    r = b * K1 + k
    return (r % B) * K1 + r // B


def _key_row_of(b, k, B, K1):
    """its inverse as the sums kernel writes it: descriptor row (b, k) -> the key row (hb, hk) that read it"""
    r = k * B + b
    return r // K1, r % K1


@pytest.mark.parametrize("B", range(1, 8))
@pytest.mark.parametrize("K1", range(1, 9))
def test_key_row_closed_form_equals_the_reference_bookkeeping(B, K1):
    rows = torch.arange(B * K1, dtype=torch.float64).view(B, K1, 1)                  # every descriptor holds its own row number
    keys = R.compat_keys(rows, True)
    for b in range(B):
        for k in range(K1):
            assert int(keys[b, k, 0]) == _key_src_row(b, k, B, K1)
            hb, hk = _key_row_of(b, k, B, K1)
            assert 0 <= hb < B and 0 <= hk < K1 and _key_src_row(hb, hk, B, K1) == b * K1 + k
    # the gather of the gradients: key-row gradients that hold their own key-row number land on the descriptor that fed them
    back = R._unkeys(torch.arange(B * K1, dtype=torch.float64).view(B, K1, 1), True)
    for b in range(B):
        for k in range(K1):
            hb, hk = _key_row_of(b, k, B, K1)
            assert int(back[b, k, 0]) == hb * K1 + hk
    assert torch.equal(R.compat_keys(rows, False), rows)


def test_retrieval_restatement_equals_normalize_einsum():
    f1, f2 = R.normal_pair(33, 41, 36)
    f1[1, 5] = 0                                                                     # a zero row: the clamp, not a NaN
    n1, n2 = F.normalize(f1.double(), dim=-1, eps=1e-12), F.normalize(f2.double(), dim=-1, eps=1e-12)
    want = torch.einsum("inc,jmc->ijnm", n1, n2).amax(dim=-1).mean(dim=-1)
    got = R.retrieval(f1, f2)
    assert got.shape == (2, 3) and bool(torch.isfinite(got).all())
    assert (got - want).abs().max().item() < TOL


@pytest.mark.parametrize("n1,n2,C", R.RETRIEVAL_CASES)
def test_negative_pairs_have_negative_scores(n1, n2, C):
    """What the negative-maximum cases of the GPU suite rely on: every score < 0 (a padded row, cos = 0, would win every maximum),
    and with one all-zero candidate point every score is exactly 0."""
    f1, f2 = R.negative_pair(n1, n2, C)
    r = R.retrieval(f1, f2)
    assert r.max().item() < -0.1, r.max().item()
    f2 = f2.clone()
    f2[:, n2 // 2] = 0
    assert bool((R.retrieval(f1, f2) == 0).all())


@pytest.mark.parametrize("C", R.RAGGED_CS)
def test_ragged_negative_pairs_have_negative_scores(C):
    qs, ks = R.ragged_shapes(C, negative=True)
    assert [q.shape[0] for q in qs] == R.RAGGED_LENS[0] and [k.shape[0] for k in ks] == R.RAGGED_LENS[1]
    for q in qs:
        for k in ks:
            assert R.retrieval(q[None], k[None]).item() < -0.1


def test_case_lists_cover_what_they_claim():
    nps = {c[3] for c in R.MIX_CASES}
    assert nps == {4, 1020, 1024, 1028, 2052}
    assert {c[3] for c in R.MIX_CASES if c[1] == 8} == nps                           # every NP with K1 = 8
    assert {c[1] for c in R.MIX_CASES if c[3] == 1028} == {1, 2, 5, 8}               # every K1 with NP = 1028
    assert {c[2] for c in R.MIX_CASES} == {1, 3, 40} and {c[0] for c in R.MIX_CASES} == {1, 3}
    k1s = {c[1] for c in R.COMPAT_CASES}
    assert k1s | {3, 4, 5, 8} == set(range(1, 9))                                   # with test_gpu_kernels.py::test_compat_head
    assert {1, 2, 6, 7} <= k1s
    assert any(c[2] < 16 for c in R.COMPAT_CASES) and any(c[2] > 16 and c[2] % 16 for c in R.COMPAT_CASES)
    assert any(c[4] for c in R.COMPAT_CASES)
    assert {c[2] for c in R.RETRIEVAL_CASES} == set(R.RETRIEVAL_CS)
    assert {c[:2] for c in R.RETRIEVAL_CASES} == set(R.RETRIEVAL_NS)
