"""The ragged cross-shape head kernels on the MI355X (csn_amd/csrc/minkowski_csn.hip; include/csn_hip.h section 11) through the raw
C ABI, against the float64 restatements of tests/ragged_head_ref.py, at the counts where their vectors, tiles and strides change:

  pool            E = 12 evaluations of 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028 points (the 4-point vector, the
                  1024-point stride of the loop) at ld = 1028 and 2052, evaluation stride C ld and C ld + 12, C in {1, 5, 64},
                  ``mean`` given and NULL
  pool backward   the same maps, accumulate 0 and 1 (ld = 2052: a grid block wholly past every count), and the call on the
                  sub-range of evaluations [3, 8) that ``_RaggedHead.backward`` makes
  mix forward     shapes of 1, 63, 64, 65, 129, 4 points (and one shape of 130) at ld = 132, 192, 260; (k1, cross_first) = (1, any),
  and backward    (2, B), (3, 3B) (the head's own layout), (8, B + 3) (unmixed evaluations in between), two more evaluations than the
                  last mixed one; C in {4, 60, 64, 68, 256}; out / dout the column slice [:, C:2C] of rows of pitch 2C + 4, and
                  plain rows of pitch C
  the node        ``_RaggedHead`` on synthetic maps with the plan of ``SimCSNHead.forward``: B = 3 shapes of 5, 65, 130 points,
                  C = 128, K = 0 (with and without ``ssa_only``), 1 and 3, against float64 autograd of the restated pool, linear_q /
                  linear_k, normalize, sim, softmax and mix

Every map holds +-1e30 from its evaluation's count to ld (FINITE: the mix backward forms 0 * xhat there), so the use of one point
at or past a count is an error of order 1e27; every stride padding, every column outside a slice and every buffer's end holds a
canary.  The kernels are fp32 elementwise with fp64 sums in a fixed order, and the math mode does not reach them: each case runs
in mode 0 and in mode 1 and the two runs must agree bit for bit.  The bounds are computed from that arithmetic (u = 2^-24), the
restatement supplies the scale:

  pooled, mean    |err| <= 2 u |ref| + 1e-12                       an fp64 sum rounded once to fp32
  pool backward   |err| <= 2 u (|prev| + |g|), n < count           g = gamma dpooled / count rounded once, one addition; exactly 0
                                                                   (accumulate 0) or the previous bits (1) from the count to ld
  mix forward     |err| <= 2 (k1 + 2) u A                          A = |gamma| sum_j |comp_j xhat_j| + |beta| sum_j |comp_j|: k1 fma,
                                                                   k1 - 1 for the sum of comp, one for beta times it, the last fma;
                                                                   a factor 2 over the first-order bound
  dxhat           |err| <= 3 u |ref|, n < length; exactly 0 from the length to ld; canary where no (b, j) maps
  rowdot, rowsum  |err| <= 2^-40 sum |d x|, 2^-40 sum |d|          fp64 sums of exact products; finite although ws starts as nan
  the node        outputs within 1e-4 absolute, every gradient within 1e-4 of its tensor's max (the project's contract, the bound
                  of tests/test_gpu_minkowski_csn.py: an error of the glue is of order 1)

Every test prints its worst error / bound (``[ragged] ...`` under ``pytest -s``).

Measured on MI355X (the same bits in both math modes), worst error / bound over all cases: pooled 0.49, mean 0.49, pool backward
0.79, mix forward 0.32, dxhat 0.66, rowdot 2.4e-4, rowsum 0 (exact).  The node: out 3.4e-7 absolute; relative to each tensor's max
dxhat 1.2e-7, dgamma 4.3e-8, dbeta 5.2e-8, dq 0 (a copy), dwq 4.6e-7, dwk 3.8e-7."""
import functools

import pytest
import torch

from tests import ragged_head_ref as R

pytestmark = pytest.mark.gpu

CANARY = R.CANARY
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


def _in_both_modes(L, fn):
    """[fn() in math mode 0, fn() in math mode 1]"""
    lib = L.lib()
    try:
        out = []
        for mode in (0, 1):
            L.check(lib.csn_set_math_mode(mode))
            out.append(fn())
        return out
    finally:
        lib.csn_set_math_mode(1)


def _dev(buf, dtype=torch.float32):
    """A flat CPU buffer on the device with GUARD canaries behind it."""
    return torch.cat([buf.to(dtype), torch.full((GUARD,), CANARY, dtype=dtype)]).cuda()


def _filled(n, fill, dtype=torch.float32):
    """n elements of ``fill`` on the device with GUARD canaries behind them."""
    buf = torch.full((n + GUARD,), CANARY, dtype=dtype, device="cuda")
    buf[:n] = fill
    return buf


def _guard_intact(*bufs):
    return all(bool((b[-GUARD:] == CANARY).all()) for b in bufs)


def _i32(values):
    h = torch.tensor(list(values), dtype=torch.int32)
    return h, h.cuda()


def _ratio(got, ref, bound):
    """max |got - ref| / bound, elementwise, in float64 on the host (a zero bound admits a zero error only)"""
    err = (got.detach().cpu().double() - ref).abs()
    return (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------
# pool
# ---------------------------------------------------------------------------------------------------------
POOL_FORMS = [(ld, pad) for ld in R.POOL_LDS for pad in (0, 3)]


@functools.lru_cache(maxsize=None)
def _pool_case(C, ld, pad):
    """Inputs and float64 results of one pool case, shared and never modified."""
    t = R.pool_inputs(C, ld, pad)
    x = R.maps(t["buf"], len(R.POOL_COUNTS), C, ld, t["stride"])
    pooled, mean, _ = R.pool(x, R.POOL_COUNTS, t["gamma"], t["beta"])
    return t, pooled, mean


def _pool_run(L, t, C, ld, want_mean):
    E = len(R.POOL_COUNTS)
    xbuf = _dev(t["buf"])
    ch, cd = _i32(R.POOL_COUNTS)
    gamma, beta = t["gamma"].cuda(), t["beta"].cuda()
    pooled, mean = _filled(E * C, CANARY), _filled(E * C, CANARY)
    L.check(L.lib().csn_ragged_pool_f32(xbuf.data_ptr(), t["stride"], ld, ch.data_ptr(), cd.data_ptr(), E, C, gamma.data_ptr(),
                                        beta.data_ptr(), pooled.data_ptr(), mean.data_ptr() if want_mean else None, _stream()),
            "csn_ragged_pool_f32")
    torch.cuda.synchronize()
    assert _guard_intact(pooled, mean) and torch.equal(xbuf.cpu()[:-GUARD], t["buf"])
    if not want_mean:
        assert bool((mean == CANARY).all())
    return pooled[:E * C].view(E, C).cpu(), mean[:E * C].view(E, C).cpu()


@pytest.mark.parametrize("C", R.POOL_CS)
def test_pool_raw_abi(L, C):
    worst = 0.0
    for ld, pad in POOL_FORMS:
        t, pooled, mean = _pool_case(C, ld, pad)
        (got, got_mean), (again, again_mean) = _in_both_modes(L, lambda: _pool_run(L, t, C, ld, True))
        only, _ = _pool_run(L, t, C, ld, False)
        rp = _ratio(got, pooled, 2 * U * pooled.abs() + 1e-12)
        rm = _ratio(got_mean, mean, 2 * U * mean.abs() + 1e-12)
        print(f"[ragged] pool C {C} ld {ld} pad {pad}: pooled {rp:.2f} mean {rm:.2f} of the bound")
        assert torch.isfinite(got).all() and torch.isfinite(got_mean).all()
        assert rp <= 1.0 and rm <= 1.0, (ld, pad, rp, rm)
        assert torch.equal(got, again) and torch.equal(got_mean, again_mean) and torch.equal(got, only)
        worst = max(worst, rp, rm)
    print(f"[ragged] pool C {C}: worst {worst:.2f} of the bound")


def _pool_bwd_run(L, t, C, ld, accumulate, first=0, n=None):
    """csn_ragged_pool_bwd_f32 on the evaluations [first, first + n) of a buffer that holds ``prev``: the whole buffer back."""
    E = len(R.POOL_COUNTS)
    n = E - first if n is None else n
    dbuf = _dev(t["prev"])
    ch, cd = _i32(R.POOL_COUNTS)
    gamma, dpooled = t["gamma"].cuda(), t["dpooled"].cuda().contiguous()
    L.check(L.lib().csn_ragged_pool_bwd_f32(dpooled[first:].data_ptr(), gamma.data_ptr(), ch[first:].data_ptr(), cd[first:].data_ptr(), n,
                                            C, dbuf.data_ptr() + 4 * first * t["stride"], t["stride"], ld, accumulate, _stream()),
            "csn_ragged_pool_bwd_f32")
    torch.cuda.synchronize()
    assert _guard_intact(dbuf)
    return dbuf.cpu()[:-GUARD]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", R.POOL_CS)
def test_pool_backward_raw_abi(L, C, accumulate):
    E, counts = len(R.POOL_COUNTS), R.POOL_COUNTS
    worst = 0.0
    for ld, pad in POOL_FORMS:
        t, _, _ = _pool_case(C, ld, pad)
        stride = t["stride"]
        prev = R.maps(t["prev"], E, C, ld, stride)
        ref, g = R.pool_bwd(t["dpooled"], t["gamma"], counts, ld, prev if accumulate else None)
        buf, again = _in_both_modes(L, lambda: _pool_bwd_run(L, t, C, ld, accumulate))
        got = R.maps(buf, E, C, ld, stride)
        assert torch.equal(buf, again)
        assert bool((R.padding(buf, E, C, ld, stride) == CANARY).all())
        r = 0.0
        for e, n in enumerate(counts):
            bound = 2 * U * ((prev[e, :, :n].double().abs() if accumulate else 0.0) + g[e].abs()[:, None].expand(C, n))
            r = max(r, _ratio(got[e, :, :n], ref[e, :, :n], bound))
            # from the count to ld: zero, or the bits that were there
            assert torch.equal(got[e, :, n:], prev[e, :, n:] if accumulate else torch.zeros(C, ld - n)), (ld, pad, e)
        print(f"[ragged] pool bwd C {C} acc {accumulate} ld {ld} pad {pad}: {r:.2f} of the bound")
        assert r <= 1.0, (ld, pad, r)
        worst = max(worst, r)
        # the sub-range call of _RaggedHead.backward: the evaluations around it keep their bits, its own get those of the whole call
        first, n_sub = R.POOL_SUB
        sub = R.maps(_pool_bwd_run(L, t, C, ld, accumulate, first, n_sub), E, C, ld, stride)
        keep = [e for e in range(E) if not first <= e < first + n_sub]
        assert torch.equal(sub[keep], prev[keep]) and torch.equal(sub[first:first + n_sub], got[first:first + n_sub])
    print(f"[ragged] pool bwd C {C} acc {accumulate}: worst {worst:.2f} of the bound")


# ---------------------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------------------
MIX_CASES = [(li, ki) for li in range(len(R.MIX_LENS)) for ki in range(4)]
MIX_IDS = [f"B{len(R.MIX_LENS[li])}-k{R.mix_layouts(len(R.MIX_LENS[li]))[ki][0]}" for li, ki in MIX_CASES]
TAIL_ROWS = 8                      # canary rows behind the last shape's


@functools.lru_cache(maxsize=None)
def _mix_case(li, ki, C, ld):
    """Inputs and float64 results of one mix case, shared and never modified."""
    lens = R.MIX_LENS[li]
    k1, cross_first = R.mix_layouts(len(lens))[ki]
    t = R.mix_inputs(lens, k1, cross_first, C, ld)
    x = R.maps(t["buf"], t["n_evals"], C, ld, t["stride"])
    out, A = R.mix_fwd(x, lens, t["comp"], t["gamma"], t["beta"], cross_first)
    return lens, k1, cross_first, t, {"out": out, "A": A, **R.mix_bwd(t["dout"], x, lens, t["comp"], t["gamma"], cross_first)}


def _rows(t, C, sliced, fill=None):
    """Point-major rows on the device, plain (pitch C) or as the columns [C, 2C) of rows of pitch 2C + 4: (flat buffer with TAIL_ROWS
    rows and a guard behind, pointer of the first row's first column, pitch).  fill None: ``dout`` inside, real values around it."""
    N = t["dout"].shape[0]
    pitch, col = (2 * C + 4, C) if sliced else (C, 0)
    if fill is None:
        rows = t["wide"][:, :pitch].clone()
        rows[:, col:col + C] = t["dout"]
        rows = torch.cat([rows, t["wide"][:TAIL_ROWS, :pitch]])
    else:
        rows = torch.full((N + TAIL_ROWS, pitch), fill)
    buf = _dev(rows.reshape(-1))
    return buf, buf.data_ptr() + 4 * col, pitch


def _mix_fwd_run(L, lens, k1, cross_first, t, C, ld, sliced):
    B, N = len(lens), sum(lens)
    xbuf = _dev(t["buf"])
    oh, od = _i32(R.offsets(lens))
    comp, gamma, beta = t["comp"].cuda().contiguous(), t["gamma"].cuda(), t["beta"].cuda()
    obuf, optr, pitch = _rows(t, C, sliced, fill=CANARY)
    L.check(L.lib().csn_ragged_mix_fwd_f32(xbuf.data_ptr(), t["stride"], ld, t["n_evals"], cross_first, oh.data_ptr(), od.data_ptr(), B,
                                           k1, C, comp.data_ptr(), gamma.data_ptr(), beta.data_ptr(), optr, pitch, _stream()),
            "csn_ragged_mix_fwd_f32")
    torch.cuda.synchronize()
    assert _guard_intact(obuf) and torch.equal(xbuf.cpu()[:-GUARD], t["buf"])
    rows = obuf.cpu()[:-GUARD].view(N + TAIL_ROWS, pitch)
    col = C if sliced else 0
    outside = torch.ones(pitch, dtype=torch.bool)
    outside[col:col + C] = False
    assert bool((rows[:, outside] == CANARY).all()) and bool((rows[N:] == CANARY).all())
    return rows[:N, col:col + C]


@pytest.mark.parametrize("C", R.MIX_CS)
@pytest.mark.parametrize("li,ki", MIX_CASES, ids=MIX_IDS)
def test_mix_forward_raw_abi(L, li, ki, C):
    worst = 0.0
    for ld in R.MIX_LDS:
        lens, k1, cross_first, t, ref = _mix_case(li, ki, C, ld)
        bound = 2 * (k1 + 2) * U * ref["A"]
        got, again = _in_both_modes(L, lambda: _mix_fwd_run(L, lens, k1, cross_first, t, C, ld, True))
        plain = _mix_fwd_run(L, lens, k1, cross_first, t, C, ld, False)
        r = _ratio(got, ref["out"], bound)
        print(f"[ragged] mix fwd lens {lens} k1 {k1} cross_first {cross_first} C {C} ld {ld}: {r:.2f} of the bound")
        assert torch.isfinite(got).all() and r <= 1.0, (ld, r)
        assert torch.equal(got, again) and torch.equal(got, plain)                  # the pitch and the mode change no bit
        worst = max(worst, r)
    print(f"[ragged] mix fwd {MIX_IDS[MIX_CASES.index((li, ki))]} C {C}: worst {worst:.2f} of the bound")


def _mix_bwd_run(L, lens, k1, cross_first, t, C, ld, sliced):
    B, E, stride = len(lens), t["n_evals"], t["stride"]
    xbuf = _dev(t["buf"])
    oh, od = _i32(R.offsets(lens))
    comp, gamma = t["comp"].cuda().contiguous(), t["gamma"].cuda()
    dbuf, dptr, pitch = _rows(t, C, sliced)
    dxbuf = _filled(E * stride, CANARY)
    ws_n = B * (k1 + 1) * ((ld + 63) // 64) * C
    ws = _filled(ws_n, float("nan"), torch.float64)
    rowdot, rowsum = _filled(B * k1 * C, float("nan"), torch.float64), _filled(B * C, float("nan"), torch.float64)
    L.check(L.lib().csn_ragged_mix_bwd_f32(dptr, pitch, xbuf.data_ptr(), stride, ld, E, cross_first, oh.data_ptr(), od.data_ptr(), B, k1, C,
                                           comp.data_ptr(), gamma.data_ptr(), dxbuf.data_ptr(), rowdot.data_ptr(), rowsum.data_ptr(),
                                           ws.data_ptr(), ws_n, _stream()), "csn_ragged_mix_bwd_f32")
    torch.cuda.synchronize()
    assert _guard_intact(dxbuf, ws, rowdot, rowsum, dbuf) and torch.equal(xbuf.cpu()[:-GUARD], t["buf"])
    return {"dxbuf": dxbuf.cpu()[:-GUARD], "rowdot": rowdot[:-GUARD].view(B, k1, C).cpu(), "rowsum": rowsum[:-GUARD].view(B, C).cpu()}


@pytest.mark.parametrize("C", R.MIX_CS)
@pytest.mark.parametrize("li,ki", MIX_CASES, ids=MIX_IDS)
def test_mix_backward_raw_abi(L, li, ki, C):
    worst = {"dxhat": 0.0, "rowdot": 0.0, "rowsum": 0.0}
    for ld in R.MIX_LDS:
        lens, k1, cross_first, t, ref = _mix_case(li, ki, C, ld)
        B, E, stride = len(lens), t["n_evals"], t["stride"]
        got, again = _in_both_modes(L, lambda: _mix_bwd_run(L, lens, k1, cross_first, t, C, ld, True))
        plain = _mix_bwd_run(L, lens, k1, cross_first, t, C, ld, False)
        for key in got:
            assert torch.equal(got[key], again[key]) and torch.equal(got[key], plain[key]), key
        dx = R.maps(got["dxbuf"], E, C, ld, stride)
        assert bool((R.padding(got["dxbuf"], E, C, ld, stride) == CANARY).all())
        assert bool((dx[~ref["written"]] == CANARY).all())                           # evaluations that no (b, j) maps to
        r = {"dxhat": 0.0}
        for b, n in enumerate(lens):
            for j in range(k1):
                e = R.ev(b, j, B, cross_first)
                r["dxhat"] = max(r["dxhat"], _ratio(dx[e, :, :n], ref["dxhat"][e, :, :n], 3 * U * ref["dxhat"][e, :, :n].abs()))
                # from the shape's points to ld: zero (a row of the next shape's dout must not appear there)
                assert not dx[e, :, n:].any(), (ld, b, j)
        assert torch.isfinite(got["rowdot"]).all() and torch.isfinite(got["rowsum"]).all()
        r["rowdot"] = _ratio(got["rowdot"], ref["rowdot"], 2.0 ** -40 * ref["dot_abs"])
        r["rowsum"] = _ratio(got["rowsum"], ref["rowsum"], 2.0 ** -40 * ref["sum_abs"])
        print(f"[ragged] mix bwd lens {lens} k1 {k1} cross_first {cross_first} C {C} ld {ld}: " +
              " ".join(f"{k} {v:.2g}" for k, v in r.items()) + " of the bound")
        assert max(r.values()) <= 1.0, (ld, r)
        worst = {k: max(worst[k], v) for k, v in r.items()}
    print(f"[ragged] mix bwd {MIX_IDS[MIX_CASES.index((li, ki))]} C {C}: worst " + " ".join(f"{k} {v:.2g}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------
# the node
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _node_case(K, ssa_only):
    """Inputs, and the float64 output and gradients of one node case by autograd of the restatement."""
    t = R.node_inputs(K)
    C = R.NODE_C
    names = ["xhat", "gamma", "beta", "q_rows"] + (["wq", "wk"] if K > 0 and not ssa_only else [])
    leaf = {n: t[n].double().clone().requires_grad_() for n in names}
    out = R.head(leaf["xhat"], leaf["q_rows"], R.NODE_LENS, t["counts"], K, ssa_only, leaf["gamma"], leaf["beta"], leaf.get("wq"),
                 leaf.get("wk"), float(C) ** 0.5)
    dout = t["dout"][:, :C] if ssa_only else t["dout"]
    grads = torch.autograd.grad((out * dout.double()).sum(), [leaf[n] for n in names], allow_unused=True)
    return t, dout, out.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("K,ssa_only", R.NODE_CASES, ids=[f"K{K}{'-ssa' if s else ''}" for K, s in R.NODE_CASES])
def test_ragged_head_node_against_float64_autograd(L, K, ssa_only):
    from csn_amd.minkowski_attention import ScaledDotProduct
    from csn_amd.minkowski_csn import _RaggedHead, _int32_pair
    t, dout, ref_out, ref = _node_case(K, ssa_only)
    C, B, dev = R.NODE_C, len(R.NODE_LENS), torch.device("cuda")

    def run():
        leaf = {n: t[n].to(dev).contiguous().requires_grad_() for n in ("xhat", "gamma", "beta", "q_rows")}
        if K > 0:
            leaf["wq"], leaf["wk"] = (t[n].to(dev).requires_grad_() for n in ("wq", "wk"))
            wq, wk = leaf["wq"], leaf["wk"]
        else:
            wq = wk = leaf["gamma"].detach().new_empty(0)
        # the plan of SimCSNHead.forward
        plan = {"B": B, "K": K, "ssa_only": ssa_only, "cross_first": B + K * B, "offsets": _int32_pair(R.offsets(R.NODE_LENS), dev),
                "counts": _int32_pair(t["counts"], dev), "sim": ScaledDotProduct(C ** 0.5)}
        out = _RaggedHead.apply(leaf["xhat"], leaf["gamma"], leaf["beta"], wq, wk, leaf["q_rows"], plan)
        out.backward(dout.to(dev))
        torch.cuda.synchronize()
        return out.detach().cpu(), {n: (v.grad.cpu() if v.grad is not None else None) for n, v in leaf.items()}

    for mode, (out, grads) in enumerate(_in_both_modes(L, run)):
        e = {"out": (out.double() - ref_out).abs().max().item()}
        for n, want in ref.items():
            if want is None:                                           # ssa_only: q does not reach the output
                assert grads[n] is None or not grads[n].any(), n
                continue
            assert grads[n] is not None and torch.isfinite(grads[n]).all(), n
            e["d" + n] = (grads[n].double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
        if K > 0 and not ssa_only:
            assert {"dwq", "dwk"} <= set(e)
        print(f"[ragged] node mode {mode} K {K} ssa_only {ssa_only}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert out.shape == ref_out.shape and torch.isfinite(out).all() and max(e.values()) < 1e-4, e
        # from every evaluation's count to ld the gradient map is zero
        for ev, n in enumerate(t["counts"]):
            assert not grads["xhat"][ev, :, n:].any(), ev
