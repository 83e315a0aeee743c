"""The kernels that close a cross-shape-attention step on the MI355X, at the shapes where their loops and tiles change, against
the float64 restatements of tests/tail_ref.py: the compatibility-weighted mix with its reductions and the row sums
(csn_amd/csrc/combine.hip), the compatibility head (csrc/compat.hip) and the retrieval measure (csrc/retrieval.hip; fixed-length
form, and the ragged form at the channel counts it was never run at).  Raw C ABI wherever a form cannot be reached through
``csn_amd.functional``; every output is carved out of a buffer of canaries with a guard behind it.  All of it is plain fp32 /
fp64 arithmetic in a fixed order (there is no second arithmetic here: the math mode does not reach these kernels, which the mix
tests assert bit for bit), so the bounds are computed, not chosen (u = 2^-24):

  feats             |err| <= (K1 + 4) u (|gamma| sum_k |comp_k xhat_k| + |beta| sum_k |comp_k|)
  dxhat             |err| <= 3 u |ref|                              two roundings: comp_k gamma, then times dfeats
  rowdot, rowsum,   |err| <= u |ref| + NP 2^-52 sum |terms|         exact products added in fp64, one rounding to fp32
  csn_rowsum_f32
  dcomp, dgamma,    |err| <= 4 u sum |terms|                        the terms of tail_ref.mix_param_grads: fp32 reductions
  dbeta                                                             combined in fp64, one rounding to fp32
  comp              2e-6 absolute, rows sum to 1 within 1e-6; each gradient of the head within 2e-5 of its tensor's maximum
                    (the bounds of test_gpu_kernels.py::test_compat_head); K1 = 1: comp == 1 and every gradient == 0 exactly;
                    C = 1: every gradient is exactly zero but for a cancellation's rounding (tail_ref.compat_scalar_tol)
  retrieval score   |err| <= (C + n1 / 256 + 32) u                  an fp32 dot product of C terms between unit-scale vectors; two
                    norms, two reciprocals, two scalings; the 256-way strided sum and the tree of the mean (the maximum is
                    1-Lipschitz, so near-ties need no exclusion)

Every test prints its worst error / bound (``[tail] ...`` under ``pytest -s``).

Measured on MI355X, worst error / bound per section: not measured."""
import functools
import math

import pytest
import torch

from tests import tail_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
GUARD = 64
U = R.U


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _carve(shape, dtype=torch.float32):
    """An output of ``shape`` full of canaries, GUARD more behind its last element: (view, whole buffer)."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), CANARY, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf


def _guard_intact(*bufs):
    return all(bool((b[-GUARD:] == CANARY).all()) for b in bufs if b is not None)


def _untouched(buf):
    return bool((buf == CANARY).all())


def _ratio(got, ref, bound):
    """max |got - ref| / bound, elementwise, in float64 on the host (a zero bound admits a zero error only)"""
    err = (got.detach().cpu().double() - ref).abs()
    return (err / bound.clamp_min(1e-300)).max().item()


def _same_bits(a, b):
    return all(torch.equal(a[n], b[n]) for n in a if a[n] is not None and b.get(n) is not None)


# ---------------------------------------------------------------------------------------------------------
# the mix and the row sums
# ---------------------------------------------------------------------------------------------------------
MIX_FORMS = [(c, f) for c in R.MIX_CASES for f in (("one", "split") if c[1] >= 2 else ("one", "self"))]
MIX_IDS = ["-".join(map(str, c)) + "-" + f for c, f in MIX_FORMS]


@functools.lru_cache(maxsize=None)
def _mix_ref(case, x16):
    """Inputs and float64 results of one case, shared and never modified.  x16: the maps as fp16 values, taken as exact."""
    t = R.mix_inputs(*case)
    if x16:
        t["xhat"] = t["xhat"].half().float()
    feats, f_scale = R.mix_fwd(t["xhat"], t["comp"], t["gamma"], t["beta"])
    dxhat, rowdot, rowsum, dot_abs, sum_abs = R.mix_bwd(t["dfeats"], t["xhat"], t["comp"], t["gamma"])
    return t, {"feats": feats, "f_scale": f_scale, "dxhat": dxhat, "rowdot": rowdot, "rowsum": rowsum, "dot_abs": dot_abs,
               "sum_abs": sum_abs, "grads": R.mix_param_grads(rowdot, rowsum, t["comp"], t["gamma"], t["beta"])}


def _mix_maps(t, form, x16):
    """(xhat, xhat_self) on the device in one of the ABI's three forms: all maps in one tensor; the k = 0 maps in their own;
    no tensor of others at all (K1 == 1)."""
    B, K1, C, NP = t["xhat"].shape
    put = (lambda x: x.half().cuda().contiguous()) if x16 else (lambda x: x.cuda().contiguous())
    if form == "one":
        return put(t["xhat"].reshape(B * K1, C, NP)), None
    own = put(t["xhat"][:, 0])
    return (put(t["xhat"][:, 1:].reshape(B * (K1 - 1), C, NP)) if form == "split" else None), own


def _mix_run(L, t, form, maps=True, x16=False):
    """csn_mix_fwd_f32 and csn_mix_bwd_f32 through the raw ABI: feats, dxhat as (B, K1, C, NP) (None in the reductions-only
    form), rowdot, rowsum on the host.  Guards checked here."""
    from csn_amd import functional as CF
    lib = L.lib()
    B, K1, C, NP = t["xhat"].shape
    x, xs = _mix_maps(t, form, x16)
    comp, gamma, beta, dfe = (t[n].cuda().contiguous() for n in ("comp", "gamma", "beta", "dfeats"))
    feats, fbuf = _carve((B, C, NP))
    rowdot, rdbuf = _carve((B, K1, C))
    rowsum, rsbuf = _carve((B, C))
    dx = dxbuf = dxs = dxsbuf = None
    if maps:
        # "self": a gradient tensor for maps that were not given — nothing may land in it
        dx, dxbuf = _carve(tuple(x.shape) if x is not None else (B, C, NP))
        if xs is not None:
            dxs, dxsbuf = _carve((B, C, NP))
    with CF.act16(2 if x16 else 0):
        L.check(lib.csn_mix_fwd_f32(_ptr(x), _ptr(comp), _ptr(gamma), _ptr(beta), _ptr(feats), B, K1, C, NP, _ptr(xs), _stream()),
                "csn_mix_fwd_f32")
        L.check(lib.csn_mix_bwd_f32(_ptr(dfe), _ptr(x), _ptr(comp), _ptr(gamma), _ptr(dx), _ptr(rowdot), _ptr(rowsum), B, K1, C, NP,
                                    _ptr(xs), _ptr(dxs), _stream()), "csn_mix_bwd_f32")
    torch.cuda.synchronize()
    assert _guard_intact(fbuf, rdbuf, rsbuf, dxbuf, dxsbuf)
    dxhat = None
    if maps:
        if form == "one":
            dxhat = dx.view(B, K1, C, NP)
        elif form == "split":                        # the k = 0 gradient map lands in dxhat_self
            dxhat = torch.cat((dxs.view(B, 1, C, NP), dx.view(B, K1 - 1, C, NP)), dim=1)
        else:
            assert _untouched(dxbuf)
            dxhat = dxs.view(B, 1, C, NP)
        dxhat = dxhat.cpu()
    return {"feats": feats.cpu(), "dxhat": dxhat, "rowdot": rowdot.cpu(), "rowsum": rowsum.cpu()}


def _mix_ratios(got, ref, K1, NP):
    r = {"feats": _ratio(got["feats"], ref["feats"], (K1 + 4) * U * ref["f_scale"]),
         "rowdot": _ratio(got["rowdot"], ref["rowdot"], U * ref["rowdot"].abs() + NP * 2.0 ** -52 * ref["dot_abs"]),
         "rowsum": _ratio(got["rowsum"], ref["rowsum"], U * ref["rowsum"].abs() + NP * 2.0 ** -52 * ref["sum_abs"])}
    if got["dxhat"] is not None:
        r["dxhat"] = _ratio(got["dxhat"], ref["dxhat"], 3 * U * ref["dxhat"].abs())
    return r


@pytest.mark.parametrize("case,form", MIX_FORMS, ids=MIX_IDS)
def test_mix_raw_abi(L, case, form):
    """fp32 maps, the three forms of the ABI: with gradient maps and reductions-only, twice, in both math modes."""
    B, K1, C, NP = case
    t, ref = _mix_ref(case, False)
    lib = L.lib()
    try:
        L.check(lib.csn_set_math_mode(0))
        got = _mix_run(L, t, form)
        L.check(lib.csn_set_math_mode(1))
        other_mode = _mix_run(L, t, form)
        again = _mix_run(L, t, form)
        reductions = _mix_run(L, t, form, maps=False)
    finally:
        lib.csn_set_math_mode(1)
    r = _mix_ratios(got, ref, K1, NP)
    print(f"[tail] mix {case} {form}: " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert _same_bits(got, other_mode), "math modes 0 and 1 differ"
    assert _same_bits(other_mode, again), "two calls differ"
    assert reductions["dxhat"] is None and _same_bits(got, reductions), "the reductions-only form differs from the form with maps"


@pytest.mark.parametrize("case,form", MIX_FORMS, ids=MIX_IDS)
def test_mix_fp16_maps(L, case, form):
    """The fp16-map instances of csn_mix_fwd_f32 and csn_mix_bwd_f32 (reductions only) under csn_set_thread_act16(2): the
    reference takes the fp16 values as exact, so the fp32 bounds hold unchanged."""
    B, K1, C, NP = case
    t, ref = _mix_ref(case, True)
    got = _mix_run(L, t, form, maps=False, x16=True)
    r = _mix_ratios(got, ref, K1, NP)
    print(f"[tail] mix fp16 {case} {form}: " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert _same_bits(got, _mix_run(L, t, form, maps=False, x16=True)), "two calls differ"


@pytest.mark.parametrize("x16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", R.MIX_CASES, ids=lambda c: "-".join(map(str, c)))
def test_rowsum(L, case, x16):
    """csn_rowsum_f32 over the rows of the case's maps, at the natural pitch and at a pitch of NP + 8 whose padding holds 1e4
    (fp16 has no 1e30; a padding value read would be 1e4 / sum |terms| of error)."""
    from csn_amd import functional as CF
    lib = L.lib()
    B, K1, C, NP = case
    t, _ = _mix_ref(case, x16)
    rows = t["xhat"].reshape(B * K1 * C, NP)
    ref, ref_abs = rows.double().sum(dim=1), rows.double().abs().sum(dim=1)
    bound = U * ref.abs() + NP * 2.0 ** -52 * ref_abs
    worst = 0.0
    for pad in (0, 8):
        dev = torch.full((rows.shape[0], NP + pad), 1e4, dtype=torch.float16 if x16 else torch.float32, device="cuda")
        dev[:, :NP] = rows.cuda()
        out, obuf = _carve((rows.shape[0],))
        with CF.act16(2 if x16 else 0):
            L.check(lib.csn_rowsum_f32(_ptr(dev), _ptr(out), rows.shape[0], NP, NP + pad, _stream()), "csn_rowsum_f32")
            out2, obuf2 = _carve((rows.shape[0],))
            L.check(lib.csn_rowsum_f32(_ptr(dev), _ptr(out2), rows.shape[0], NP, NP + pad, _stream()), "csn_rowsum_f32")
        torch.cuda.synchronize()
        assert _guard_intact(obuf, obuf2) and torch.equal(out, out2)
        worst = max(worst, _ratio(out, ref, bound))
    print(f"[tail] rowsum {'fp16' if x16 else 'fp32'} {case}: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case,split", [(c, s) for c in R.MIX_CASES for s in ((False, True) if c[1] >= 2 else (False,))],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else ("self-separate" if v else "one-tensor"))
def test_mix_autograd(L, case, split):
    """CF.csa_mix: d comp, d gamma and d beta are differences of large numbers; each within 4 u of the sum of |terms|."""
    from csn_amd import functional as CF
    B, K1, C, NP = case
    t, ref = _mix_ref(case, False)
    cg, gg, bg = (t[n].cuda().requires_grad_() for n in ("comp", "gamma", "beta"))
    if split:
        own = t["xhat"][:, 0].contiguous().cuda().requires_grad_()
        rest = t["xhat"][:, 1:].reshape(B * (K1 - 1), C, NP).contiguous().cuda().requires_grad_()
        got = CF.csa_mix(rest, cg, gg, bg, B, K1, xself=own)
    else:
        allm = t["xhat"].reshape(B * K1, C, NP).cuda().requires_grad_()
        got = CF.csa_mix(allm, cg, gg, bg, B, K1)
    got.backward(t["dfeats"].cuda())
    dx = torch.cat((own.grad.view(B, 1, C, NP), rest.grad.view(B, K1 - 1, C, NP)), dim=1) if split else allm.grad.view(B, K1, C, NP)
    r = {"feats": _ratio(got, ref["feats"], (K1 + 4) * U * ref["f_scale"]), "dxhat": _ratio(dx, ref["dxhat"], 3 * U * ref["dxhat"].abs())}
    for name, g, (want, terms) in zip(("dcomp", "dgamma", "dbeta"), (cg.grad, gg.grad, bg.grad), ref["grads"]):
        r[name] = _ratio(g, want, 4 * U * terms)
    print(f"[tail] mix autograd {case} {'split' if split else 'one'}: " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


# ---------------------------------------------------------------------------------------------------------
# the compatibility head
# ---------------------------------------------------------------------------------------------------------
GRADS = ("pooled", "wq", "bq", "wk", "bk")


@functools.lru_cache(maxsize=None)
def _compat_ref(B, K1, C, ref_layout, zero_row=None):
    t = R.compat_inputs(B, K1, C, zero_row=zero_row)
    comp, grads = R.compat(t["pooled"], t["wq"], t["bq"], t["wk"], t["bk"], ref_layout, t["dcomp"])
    return t, comp, grads


def _compat_raw(L, t, ref_layout):
    """csn_compat_fwd_f32 / _bwd_f32 through the raw ABI, every output (save_u, save_norm and the workspace too) carved with a
    guard: comp and the five gradients on the host."""
    lib = L.lib()
    B, K1, C = t["pooled"].shape
    pooled, wq, bq, wk, bk, dcomp = (t[n].cuda().contiguous() for n in GRADS + ("dcomp",))
    comp, cbuf = _carve((B, K1))
    save_u, ubuf = _carve((B, K1 + 1, C), torch.float64)
    save_n, nbuf = _carve((B, K1 + 1), torch.float64)
    wq_t, wk_t = wq.t().contiguous(), wk.t().contiguous()
    L.check(lib.csn_compat_fwd_f32(_ptr(pooled), _ptr(wq_t), _ptr(bq), _ptr(wk_t), _ptr(bk), _ptr(comp),
                                   _ptr(save_u), _ptr(save_n), B, K1, C, 1 if ref_layout else 0, _stream()), "csn_compat_fwd_f32")
    ws_n = 2 * B * (K1 + 1) * C
    ws, wbuf = _carve((ws_n,), torch.float64)
    outs = {n: _carve(tuple(t[n].shape)) for n in GRADS}
    L.check(lib.csn_compat_bwd_f32(_ptr(dcomp), _ptr(comp), _ptr(save_u), _ptr(save_n), _ptr(pooled), _ptr(wq), _ptr(wk), _ptr(ws), ws_n,
                                   *[_ptr(outs[n][0]) for n in GRADS], B, K1, C, 1 if ref_layout else 0, _stream()),
            "csn_compat_bwd_f32")
    torch.cuda.synchronize()
    assert _guard_intact(cbuf, ubuf, nbuf, wbuf, *[outs[n][1] for n in GRADS])
    assert not bool((save_u == CANARY).any()) and not bool((save_n == CANARY).any())
    return comp.cpu(), {n: outs[n][0].cpu() for n in GRADS}


def _compat_autograd(t, ref_layout):
    from csn_amd import functional as CF
    a = {n: t[n].cuda().clone().requires_grad_(True) for n in GRADS}
    comp = CF.compat_head(*[a[n] for n in GRADS], reference_layout=ref_layout)
    comp.backward(t["dcomp"].cuda())
    torch.cuda.synchronize()
    return comp.detach().cpu(), {n: a[n].grad.cpu() for n in GRADS}


def _rel(got, want):
    return ((got.double() - want).abs().max() / want.abs().max()).item()


@pytest.mark.parametrize("B,K1,C,ref_layout,beyond", R.COMPAT_CASES)
def test_compat_head_edges(L, B, K1, C, ref_layout, beyond):
    """comp and all five gradients at channel counts that run the scalar tail loops alone (C < 16), the unrolled loop plus the
    tail, C either side of a wave, the K1 instances 1, 2, 6 and 7, and B*K1*C > C*C (``beyond``: the dpooled threads past the
    weight threads of the sums kernel).  Bounds: those of test_gpu_kernels.py::test_compat_head."""
    t, c64, g64 = _compat_ref(B, K1, C, ref_layout)
    comp, grads = _compat_raw(L, t, ref_layout)
    comp_ag, grads_ag = _compat_autograd(t, ref_layout)
    assert torch.equal(comp, comp_ag) and _same_bits(grads, grads_ag), "raw ABI and CF.compat_head differ"
    _, again = _compat_raw(L, t, ref_layout)
    assert _same_bits(grads, again), "two backward calls differ"
    assert (B * K1 * C > C * C) == beyond
    e_comp = (comp.double() - c64).abs().max().item()
    e_sum = (comp.double().sum(dim=1) - 1).abs().max().item()
    if K1 == 1:                                      # nothing to choose between: exact, and compared absolutely (the reference is zero)
        worst = max(grads[n].abs().max().item() for n in GRADS)
        print(f"[tail] compat {(B, K1, C, ref_layout)}: comp - 1 {e_comp:.1e}  max |grad| {worst:.1e}")
        assert bool((comp == 1).all()) and worst == 0.0
        return
    if C == 1:                                       # exactly zero but for a cancellation's rounding: an absolute bound
        tol = R.compat_scalar_tol(*[t[n] for n in GRADS], ref_layout, t["dcomp"])
        e = {n: grads[n].abs().max().item() / tol for n in GRADS}
    else:
        e = {n: _rel(grads[n], g64[n]) / 2e-5 for n in GRADS}
    print(f"[tail] compat {(B, K1, C, ref_layout)}: comp {e_comp / 2e-6:.3f}  rows {e_sum / 1e-6:.3f}  "
          + "  ".join(f"d{n} {v:.4f}" for n, v in e.items()))
    assert e_comp < 2e-6 and e_sum < 1e-6
    assert all(v < 1.0 for v in e.values()), e


@pytest.mark.parametrize("B,K1,C,ref_layout,zero_row", R.COMPAT_DEGENERATE)
def test_compat_head_zero_norm_key(L, B, K1, C, ref_layout, zero_row):
    """One key descriptor all zeros and bk = 0: its projected key is exactly zero and takes the ``norm <= eps`` branch, where the
    division is by the constant 1e-12.  That row of dpooled and dbk are about 1e11 to 1e12 and are compared relative to their own
    maxima; the other rows of dpooled, dwq, dbq and dwk relative to theirs (one maximum over all of dpooled would hide them)."""
    t, c64, g64 = _compat_ref(B, K1, C, ref_layout, zero_row)
    comp, grads = _compat_raw(L, t, ref_layout)
    comp_ag, grads_ag = _compat_autograd(t, ref_layout)
    assert torch.equal(comp, comp_ag) and _same_bits(grads, grads_ag)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    b0, k0 = zero_row
    keep = torch.ones(B, K1, dtype=torch.bool)
    keep[b0, k0] = False
    e = {"row": _rel(grads["pooled"][b0, k0], g64["pooled"][b0, k0]), "rest": _rel(grads["pooled"][keep], g64["pooled"][keep]),
         "wq": _rel(grads["wq"], g64["wq"]), "bq": _rel(grads["bq"], g64["bq"]), "wk": _rel(grads["wk"], g64["wk"]),
         "bk": _rel(grads["bk"], g64["bk"])}
    e_comp = (comp.double() - c64).abs().max().item()
    print(f"[tail] compat zero-norm key {(B, K1, C, ref_layout)}: comp {e_comp / 2e-6:.3f}  "
          + "  ".join(f"{n} {v / 2e-5:.4f}" for n, v in e.items()))
    assert g64["pooled"][b0, k0].abs().max().item() > 1e10 and g64["pooled"][keep].abs().max().item() < 1e3
    assert e_comp < 2e-6 and all(v < 2e-5 for v in e.values()), e


# ---------------------------------------------------------------------------------------------------------
# the retrieval measure
# ---------------------------------------------------------------------------------------------------------
def _retrieval_raw(L, f1, f2):
    """csn_retrieval_measure_f32 with ``out`` and the workspace carved: (S1, S2) on the host."""
    S1, N1, C = f1.shape
    S2, N2, _ = f2.shape
    a, b = f1.cuda().contiguous(), f2.cuda().contiguous()
    out, obuf = _carve((S1, S2))
    ws_n = S1 * N1 + S2 * N2 + S1 * S2 * N1
    ws, wbuf = _carve((ws_n,))
    L.check(L.lib().csn_retrieval_measure_f32(_ptr(a), _ptr(b), _ptr(out), S1, N1, S2, N2, C, _ptr(ws), ws_n, _stream()),
            "csn_retrieval_measure_f32")
    torch.cuda.synchronize()
    assert _guard_intact(obuf, wbuf)
    return out.cpu()


@pytest.mark.parametrize("kind", ["normal", "negative"])
@pytest.mark.parametrize("n1,n2,C", R.RETRIEVAL_CASES)
def test_retrieval_fixed_form_edges(L, n1, n2, C, kind):
    """Query and candidate counts around the 128-row tile, channel counts that are no multiple of the 32-channel slab (and below
    a wave of the norm kernel); ``negative``: every cosine < 0, so a padded row in the maximum (cos = 0) would win it."""
    from csn_amd import functional as CF
    f1, f2 = (R.normal_pair if kind == "normal" else R.negative_pair)(n1, n2, C)
    want = R.retrieval(f1, f2)
    if kind == "negative":
        assert want.max().item() < -0.1
    got = _retrieval_raw(L, f1, f2)
    ratio = (got.double() - want).abs().max().item() / R.retrieval_bound(C, n1)
    print(f"[tail] retrieval {kind} {(n1, n2, C)}: {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got, CF.retrieval_measure(f1.cuda(), f2.cuda()).cpu())
    assert torch.equal(got, _retrieval_raw(L, f1, f2)), "two calls differ"


@pytest.mark.parametrize("n1,n2,C", R.RETRIEVAL_CASES)
def test_retrieval_zero_points(L, n1, n2, C):
    """Among negative candidates one all-zero candidate point is every query point's maximum: every score is exactly 0, as the
    clamp-normalised zero row of the reference gives.  One all-zero query point contributes exactly 0 to the mean."""
    f1, f2 = R.negative_pair(n1, n2, C)
    z2 = f2.clone()
    z2[:, n2 // 2] = 0
    assert bool((R.retrieval(f1, z2) == 0).all())
    got = _retrieval_raw(L, f1, z2)
    assert bool((got == 0).all()), got
    z1 = f1.clone()
    z1[:, n1 // 2] = 0
    want = R.retrieval(z1, f2)
    got = _retrieval_raw(L, z1, f2)
    ratio = (got.double() - want).abs().max().item() / R.retrieval_bound(C, n1)
    print(f"[tail] retrieval zero query point {(n1, n2, C)}: {ratio:.3f}")
    assert ratio <= 1.0
    if n1 == 1:
        assert bool((got == 0).all())


def _pack(shapes):
    off = [0]
    for s in shapes:
        off.append(off[-1] + s.shape[0])
    return torch.cat(shapes).cuda().contiguous(), off


@pytest.mark.parametrize("kind", ["normal", "negative"])
@pytest.mark.parametrize("C", R.RAGGED_CS)
def test_ragged_retrieval_channel_edges(L, C, kind):
    """The ragged form at channel counts with a short last slab, lengths 1 / 127 / 129 against 128 / 130: the bound of the
    fixed form with each query shape's own point count."""
    from csn_amd.minkowski_csn import retrieval_measure_ragged
    qs, ks = R.ragged_shapes(C, negative=(kind == "negative"))
    f1, o1 = _pack(qs)
    f2, o2 = _pack(ks)
    got = retrieval_measure_ragged(f1, o1, f2, o2).cpu()
    want = torch.stack([torch.stack([R.retrieval(q[None], k[None])[0, 0] for k in ks]) for q in qs])
    if kind == "negative":
        assert want.max().item() < -0.1
    bound = torch.tensor([R.retrieval_bound(C, q.shape[0]) for q in qs], dtype=torch.float64)[:, None].expand_as(want)
    ratio = _ratio(got, want, bound)
    print(f"[tail] ragged retrieval {kind} C={C}: {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got, retrieval_measure_ragged(f1, o1, f2, o2).cpu())


@pytest.mark.parametrize("C", R.RAGGED_CS)
def test_ragged_retrieval_equals_fixed_form(L, C):
    from csn_amd import functional as CF
    from csn_amd.minkowski_csn import retrieval_measure_ragged
    f1, f2 = R.normal_pair(129, 129, C, seed=3)
    fixed = CF.retrieval_measure(f1.cuda(), f2.cuda())
    ragged = retrieval_measure_ragged(f1.reshape(-1, C).cuda(), [i * 129 for i in range(f1.shape[0] + 1)], f2.reshape(-1, C).cuda(),
                                      [i * 129 for i in range(f2.shape[0] + 1)])
    diff = (fixed - ragged).abs().max().item()
    print(f"[tail] ragged - fixed C={C}: {diff:.1e}")
    assert diff < 1e-6
