"""The cross-length and ragged-batch attention entry points (include/csn_hip.h (3b), (3c)) at every edge, through the raw C ABI,
against the float64 reference of tests/cross_attn_ref.py: key counts that are no multiples of 4 (down to one key), more than
512 keys, query count != key count with a partial last query tile, the mask pitch max(n_queries, score_pitch), both data flows
of the mode-1 backward (fp32 P / dS rows below score_pitch = round-up-32(n_keys), bf16 tile planes from there on), ragged
batches whose counts all differ.  Errors are taken per (evaluation, head).  The padding columns of every input map hold finite
sentinels that would be an O(1) error if read as data (tests/test_cpu_cross_attn_edges.py shows that without a GPU); every
output lies inside a buffer of a NaN pattern with guards, and everything the contract leaves alone must keep the pattern.

Allowances: BOUNDS of tests/attn_edge_ref.py — (forward outputs, gradients) = (5e-6, 2e-5) in mode 0 and (2e-4, 2e-4) in mode 1.
They were set for at most 512 keys; an evaluation with more keys, and any mode-0 evaluation that exceeds them, is allowed
max(BOUNDS, 4 x err32), err32 being the distance from float64 of the same formula evaluated by torch in float32 on the CPU
from the same inputs (the factor 4: an online softmax over 32-key tiles sums in another order than torch's row-wise one).
For a mode-0 evaluation "allowed max(...) once it exceeds BOUNDS" and "allowed max(...)" are the same rule."""
import pytest
import torch

from tests import attn_edge_ref as ar
from tests import cross_attn_ref as cr

pytestmark = pytest.mark.gpu

CROSS, VARLEN = cr.cross_rows(), cr.varlen_rows()
RESCALE = 8.0


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Launch:
    """the device side of one row: input maps with sentinels in every padding element, and the four entry points"""

    def __init__(self, L, r, which=0):
        self.L, self.lib, self.r, self.sen = L, L.lib(), r, cr.SENTINELS[which]
        self.q, self.k, self.v, self.dctx = cr.cross_inputs(r, which)              # host fp32 maps
        E, D = r["E"], r["H"] * r["d"]
        self.NQ, self.NK = max(r["nq"]), max(r["nk"])
        self.varlen = r["kind"] == "varlen"

        def put(x, stride, fill):
            buf = torch.full((E, stride), fill, dtype=torch.float32, device="cuda")
            buf[:, :x.shape[1] * x.shape[2]] = x.reshape(E, -1).cuda()
            return buf

        self.qd, self.dd = put(self.q, r["q_stride"], self.sen["q"]), put(self.dctx, r["q_stride"], self.sen["dctx"])
        self.kd, self.vd = put(self.k, r["kv_stride"], self.sen["k_other"]), put(self.v, r["kv_stride"], self.sen["v"])
        self.nqd = torch.tensor(r["nq"], dtype=torch.int32, device="cuda")
        self.nkd = torch.tensor(r["nk"], dtype=torch.int32, device="cuda")
        self.w_q = cr.map_written(r, False, "cuda")
        self.w_kv = cr.map_written(r, True, "cuda")
        self.w_stat = cr.stat_written(r, "cuda")
        self.planes = cr.planes_flow(r["mode"], r["Tp"], self.NK)
        self.n_sc = E * r["H"] * self.NQ * r["Tp"]

    def counts(self):
        return (self.NQ, self.NK, self.nqd.data_ptr(), self.nkd.data_ptr()) if self.varlen else (self.NQ, self.NK)

    def fwd_rc(self, ctx, sc, lse, **over):
        r = self.r
        a = dict(E=r["E"], H=r["H"], d=r["d"], Tp=r["Tp"], ld_q=r["ld_q"], ld_kv=r["ld_kv"], counts=self.counts())
        a.update(over)
        fn = self.lib.csn_varlen_attn_fwd_f32 if self.varlen else self.lib.csn_cross_attn_fwd_f32
        return fn(self.qd.data_ptr(), self.kd.data_ptr(), self.vd.data_ptr(), r["q_stride"], r["kv_stride"], a["ld_q"], a["ld_kv"],
                  ctx.ptr, r["q_stride"], sc.ptr if sc else None, lse.ptr if lse else None, a["E"], a["H"], a["d"], *a["counts"],
                  a["Tp"], RESCALE, r["p"], r["seed"], _stream())

    def fwd(self, scores=True, lse=True):
        r = self.r
        ctx = ar.Canary(r["E"] * r["q_stride"])
        ls = ar.Canary(r["E"] * r["H"] * self.NQ) if lse else None
        sc = ar.Canary(self.n_sc) if scores else None
        self.L.check(self.fwd_rc(ctx, sc, ls), "forward")
        return ctx, ls, sc

    def clean_inputs(self, ctx, lse):
        """what a caller hands to the backward: the forward's ctx and lse with FINITE padding (the forward rightly left the NaN
        pattern there; "the padding points of the input maps must be finite" is the caller's side of the contract)"""
        c = torch.where(self.w_q.reshape(-1), ctx.f32(), torch.full_like(ctx.f32(), self.sen["ctx"]))
        s = torch.where(self.w_stat.reshape(-1), lse.f32(), torch.full_like(lse.f32(), self.sen["lse"]))
        return c, s

    def bwd_rc(self, ctx_in, lse_in, sc, ds, delta, dq, dk, dv, **over):
        r = self.r
        a = dict(d=r["d"], Tp=r["Tp"], ld_q=r["ld_q"], ld_kv=r["ld_kv"], counts=self.counts())
        a.update(over)
        fn = self.lib.csn_varlen_attn_bwd_f32 if self.varlen else self.lib.csn_cross_attn_bwd_f32
        return fn(self.dd.data_ptr(), ctx_in.data_ptr(), r["q_stride"], self.qd.data_ptr(), self.kd.data_ptr(), self.vd.data_ptr(),
                  r["q_stride"], r["kv_stride"], a["ld_q"], a["ld_kv"], sc.ptr, ds.ptr, lse_in.data_ptr(), delta.ptr, dq.ptr, dk.ptr,
                  dv.ptr, r["q_stride"], r["kv_stride"], r["E"], r["H"], a["d"], *a["counts"], a["Tp"], r["p"], r["seed"], _stream())

    def bwd(self, ctx_in, lse_in, kept_scores):
        r = self.r
        out = dict(P=kept_scores.clone(), dS=ar.Canary(self.n_sc), delta=ar.Canary(r["E"] * r["H"] * self.NQ),
                   dq=ar.Canary(r["E"] * r["q_stride"]), dk=ar.Canary(r["E"] * r["kv_stride"]), dv=ar.Canary(r["E"] * r["kv_stride"]))
        self.L.check(self.bwd_rc(ctx_in, lse_in, out["P"], out["dS"], out["delta"], out["dq"], out["dk"], out["dv"]), "backward")
        return out

    def everything(self):
        """forward with kept scores and backward: every output buffer, guards included"""
        ctx, lse, sc = self.fwd()
        out = self.bwd(*self.clean_inputs(ctx, lse), sc)
        out.update(ctx=ctx, lse=lse, S=sc)
        return out

    # ---- views of one evaluation ------------------------------------------------------------------------------------------
    def q_map(self, c, e):
        r = self.r
        return c.f32().view(r["E"], -1)[e, :r["H"] * r["d"] * r["ld_q"]].view(r["H"], r["d"], r["ld_q"])[:, :, :r["nq"][e]]

    def kv_map(self, c, e, n=None):
        r = self.r
        return c.f32().view(r["E"], -1)[e, :r["H"] * r["d"] * r["ld_kv"]].view(r["H"], r["d"], r["ld_kv"])[:, :, :n or r["nk"][e]]

    def stat(self, c, e):
        return c.f32().view(self.r["E"], self.r["H"], self.NQ)[e, :, :self.r["nq"][e]]

    def rows32(self, c, e):
        """fp32 score rows of evaluation e: (H, nq[e], Tp)"""
        return c.f32().view(self.r["E"], self.r["H"], self.NQ, self.r["Tp"])[e, :, :self.r["nq"][e]]

    def plane_rows(self, c, e):
        """mode-1 tile planes — per query row tiles of [hi 32 | lo 32] bf16, the bytes of the fp32 row — decoded: (H, nq[e], Tp)"""
        r = self.r
        x = c.body.view(torch.bfloat16).view(r["E"], r["H"], self.NQ, r["Tp"] // 32, 2, 32)[e, :, :r["nq"][e]]
        return (x[..., 0, :].float() + x[..., 1, :].float()).reshape(r["H"], r["nq"][e], r["Tp"])


def _pattern_or(x, value):
    """every element still holds the canary pattern or is `value` (compared as bits / as numbers)"""
    return bool(((x.contiguous().view(torch.int32) == ar.CANARY32) | (x == value)).all())


def _without_zero_signs(la, o):
    """the buffers of Launch.everything() as bits, with -0 turned into +0 in the padding columns.  The columns nk ..
    round-up-4(nk) of a P / dS row (nk .. round-up-32(nk) of tile planes) and of dk / dv hold zeros (test_*_attention_edges
    asserts that) which are products 0 * (a padding value): +0 or -0 with the padding's sign.  Every other bit of every
    buffer must be identical."""
    r, G = la.r, ar.GUARD
    E, H, Tp = r["E"], r["H"], r["Tp"]
    out = {n: c.buf.clone() for n, c in o.items()}

    def plus_zero(x, minus_zero):
        x[x == minus_zero] = 0

    for n in ("P", "dS"):
        for e in range(E):
            nq, nk = r["nq"][e], r["nk"][e]
            if la.planes:                                                  # tile t: [hi 32 | lo 32] 16-bit elements
                body = out[n][G:G + la.n_sc].view(torch.int16).view(E, H, la.NQ, Tp // 32, 2, 32)
                t, k0 = nk // 32, nk % 32
                if k0:
                    plus_zero(body[e, :, :nq, t, :, k0:], -2 ** 15)
            else:
                plus_zero(out[n][G:G + la.n_sc].view(E, H, la.NQ, Tp)[e, :, :nq, nk:ar.ceil_to(nk, 4)], -2 ** 31)
    D = H * r["d"]
    for n in ("dk", "dv"):
        body = out[n][G:G + E * r["kv_stride"]].view(E, r["kv_stride"])
        for e in range(E):
            nk = r["nk"][e]
            plus_zero(body[e, :D * r["ld_kv"]].view(D, r["ld_kv"])[:, nk:ar.ceil_to(nk, 4)], -2 ** 31)
    return out


def _check_row(L, r):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(r["mode"]))
    E, H, d, p = r["E"], r["H"], r["d"], r["p"]
    la = Launch(L, r)
    fb, bb = ar.BOUNDS[r["mode"]]
    f64 = lambda t: t.double().view(E, H, d, -1).cuda()
    q, k, v, dctx = f64(la.q), f64(la.k), f64(la.v), f64(la.dctx)
    keep = cr.row_keep(r)                                                   # the launch's n_queries / max_queries and pitch
    ref = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep.cuda() if keep is not None else None, p)
    cond = cr.row_condition(r, ref, q, k, v, dctx, keep)
    assert max(cond.values()) <= cr.COND_LIMIT, f"ill-conditioned draw (tests/cross_attn_ref.py REDRAW): {cond}"
    # err32: the same formula in float32 on the CPU, where the rule of the module docstring may need it
    need32 = [r["mode"] == 0 or r["nk"][e] > 512 for e in range(E)]
    ref32 = None
    if any(need32):
        c32 = lambda t: t.float().view(E, H, d, -1)
        ref32 = cr.cross_attention_ref(c32(la.q), c32(la.k), c32(la.v), c32(la.dctx), r["nq"], r["nk"], keep, p, dtype=torch.float32)
    worst, long_rows = {}, []

    def value(name, e, got):
        want = ref[e][{"dq": "dq", "dk": "dk", "dv": "dv"}.get(name, name)]
        bound = fb if name in ("ctx", "lse", "S", "P") else bb
        scale = None
        if r["nk"][e] == 1 and name in ("dS", "dq", "dk"):                 # the reference is exactly zero: the natural scale
            assert float(want.abs().max()) == 0.0
            scale = cr.zero_scales(q[e], k[e], v[e], dctx[e], r["nq"][e], 1)[name]
        err = cr.eval_err(got, want, scale)
        allow = bound
        if need32[e]:
            e32 = cr.eval_err(ref32[e][name].cuda(), want, scale)
            allow = max(bound, 4 * e32)
            if r["nk"][e] > 512:
                long_rows.append(f"{name} e{e} err32 {e32:.1e} kernel {err:.1e}")
        worst[name] = max(worst.get(name, 0.0), err / allow)
        assert err < allow, f"{name}, evaluation {e} ({r['nq'][e]} x {r['nk'][e]}): error {err:.3e} >= {allow:.2e}"

    # ---- forward: kept scores, no scores, no lse; repeatable
    ctx, lse, sc = la.fwd()
    ctx.check(la.w_q, "ctx")
    lse.check(la.w_stat, "lse")
    sc.check(cr.score_written(r, False, "cuda"), "scores")
    for e in range(E):
        nk, nk4 = r["nk"][e], ar.ceil_to(r["nk"][e], 4)
        value("ctx", e, la.q_map(ctx, e))
        value("lse", e, la.stat(lse, e))
        value("S", e, la.rows32(sc, e)[..., :nk])
        assert _pattern_or(la.rows32(sc, e)[..., nk:nk4], float("-inf")), "score columns nk .. round-up-4(nk) after the forward"
    ctx1, lse1, _ = la.fwd(scores=False)
    assert torch.equal(ctx1.buf, ctx.buf) and torch.equal(lse1.buf, lse.buf), "forward differs without kept scores"
    if 33 in r["nk"]:                                                         # (once per head width, mode and entry point)
        ctx0, _, _ = la.fwd(scores=False, lse=False)
        assert torch.equal(ctx0.buf, ctx.buf), "forward differs without lse"
    ctx2, lse2, sc2 = la.fwd()
    assert torch.equal(ctx2.buf, ctx.buf) and torch.equal(lse2.buf, lse.buf) and torch.equal(sc2.buf, sc.buf), "forward not repeatable"

    # ---- backward on a copy of the kept scores
    ctx_in, lse_in = la.clean_inputs(ctx, lse)
    g = la.bwd(ctx_in, lse_in, sc)
    sw = cr.score_written(r, la.planes, "cuda")
    g["P"].check(sw, "P")
    g["dS"].check(sw, "dS")
    g["delta"].check(la.w_stat, "delta")
    g["dq"].check(la.w_q, "dq")
    g["dk"].check(la.w_kv, "dk")
    g["dv"].check(la.w_kv, "dv")
    for e in range(E):
        nk, nk4, nk32 = r["nk"][e], ar.ceil_to(r["nk"][e], 4), ar.ceil_to(r["nk"][e], 32)
        if la.planes:
            P, dS = la.plane_rows(g["P"], e), la.plane_rows(g["dS"], e)
            assert bool((P[..., nk:nk32] == 0).all()) and bool((dS[..., nk:nk32] == 0).all()), "tile-plane padding keys are not zero"
        else:
            P, dS = la.rows32(g["P"], e), la.rows32(g["dS"], e)
            assert _pattern_or(P[..., nk:nk4], 0.0) and _pattern_or(dS[..., nk:nk4], 0.0), "P / dS columns nk .. round-up-4(nk)"
        value("P", e, P[..., :nk])
        value("dS", e, dS[..., :nk])
        value("delta", e, la.stat(g["delta"], e))
        value("dq", e, la.q_map(g["dq"], e))
        value("dk", e, la.kv_map(g["dk"], e))
        value("dv", e, la.kv_map(g["dv"], e))
        for n in ("dk", "dv"):
            assert bool((la.kv_map(g[n], e, nk4)[..., nk:] == 0).all()), f"{n}: the columns nk .. round-up-4(nk) are not exact zeros"
    g2 = la.bwd(ctx_in, lse_in, sc)
    for n in g:
        assert torch.equal(g2[n].buf, g[n].buf), f"backward not repeatable: {n}"
    print(f"[cross-edge] {cr.row_id(r)} ({'planes' if la.planes else 'rows'}): worst error / allowance "
          + " ".join(f"{n} {w:.2f}" for n, w in worst.items()))
    if long_rows:
        print(f"[cross-edge long] {cr.row_id(r)}: " + "; ".join(long_rows))


@pytest.mark.parametrize("r", CROSS, ids=[cr.row_id(r) for r in CROSS])
def test_cross_attention_edges(L, r):
    _check_row(L, r)


@pytest.mark.parametrize("r", VARLEN, ids=[cr.row_id(r) for r in VARLEN])
def test_varlen_attention_edges(L, r):
    _check_row(L, r)


@pytest.mark.parametrize("r", cr.resentinel_rows(), ids=[cr.row_id(r) for r in cr.resentinel_rows()])
def test_padding_is_not_read_as_data(L, r):
    """the same row with other sentinel values in every padding element of q, k, v, dctx, ctx, lse: every output bit-identical"""
    L.check(L.lib().csn_set_math_mode(r["mode"]))
    la, lb = Launch(L, r, 0), Launch(L, r, 1)
    assert not torch.equal(la.kd, lb.kd) and not torch.equal(la.vd, lb.vd)           # (every such row has padding keys)
    a, b = _without_zero_signs(la, la.everything()), _without_zero_signs(lb, lb.everything())
    differ = [n for n in a if not torch.equal(a[n], b[n])]
    assert not differ, f"{differ} depend on the padding of the input maps"


OTHER = cr.other_mode_rows()


@pytest.mark.parametrize("r", OTHER, ids=[cr.row_id(r) for r in OTHER])
def test_modes_2_and_3_run_as_mode_1(L, r):
    """Math modes 2 and 3 run these entry points as mode 1 — forward and backward, the backward in mode 3 included — bit for
    bit, and leave the process mode and the calling thread's override as they were, also when the call returns an error."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    la = Launch(L, r)
    want = la.everything()
    for mode, per_thread in ((2, False), (3, False), (2, True), (3, True)):
        if per_thread:
            L.check(lib.csn_set_math_mode(0))                                 # (the override, not the process mode, decides)
            L.check(lib.csn_set_thread_math_mode(mode))
        else:
            L.check(lib.csn_set_thread_math_mode(-1))
            L.check(lib.csn_set_math_mode(mode))
        state = (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode())
        assert state == (mode, mode if per_thread else -1)
        got = la.everything()
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state, "a call changed the math mode"
        for n in want:
            assert torch.equal(got[n].buf, want[n].buf), f"mode {mode}: {n} differs from the mode-1 call"
        # calls that fail behind the scoped override (no kernel instance for the head width) restore it too
        assert la.fwd_rc(got["ctx"], got["S"], got["lse"], d=40) == -5
        ci, li = la.clean_inputs(got["ctx"], got["lse"])
        assert la.bwd_rc(ci, li, got["P"], got["dS"], got["delta"], got["dq"], got["dk"], got["dv"], d=40) == -5
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state, "a failed call changed the math mode"
        for n in want:
            assert torch.equal(got[n].buf, want[n].buf), f"a refused call wrote {n}"


def test_argument_rules_of_the_cross_length_entry_points(L):
    """What tests/test_gpu_kernels.py::test_abi_argument_validation_table does not list for this path: a score pitch below
    round-up-4(n_keys) (CSN_E_ALIGN, as for the block path), and for the ragged entry points the leading dimensions below the
    maxima (CSN_E_ARG: a count beyond its row) and the whole backward: NULL count arrays, max_queries % 4."""
    ARG, ALIGN = -1, -2
    L.check(L.lib().csn_set_math_mode(0))
    for r in (dict(CROSS[30], p=0.0), dict(VARLEN[0], p=0.0)):
        la = Launch(L, r)
        o = la.everything()                                                   # the unmutated calls succeed
        ci, li = la.clean_inputs(o["ctx"], o["lse"])
        fwd = lambda **kw: la.fwd_rc(o["ctx"], o["S"], o["lse"], **kw)
        bwd = lambda **kw: la.bwd_rc(ci, li, o["P"], o["dS"], o["delta"], o["dq"], o["dk"], o["dv"], **kw)
        nk4 = ar.ceil_to(la.NK, 4)
        for call in (fwd, bwd):
            assert call(Tp=nk4 - 4) == ALIGN
            assert call(ld_kv=nk4 - 4) == ARG
            assert call(ld_q=la.NQ - 4) == ARG
            if la.varlen:
                nq, nk = la.nqd.data_ptr(), la.nkd.data_ptr()
                assert call(counts=(la.NQ, la.NK, None, nk)) == ARG
                assert call(counts=(la.NQ, la.NK, nq, None)) == ARG
                assert call(counts=(la.NQ + 2, la.NK, nq, nk)) == ALIGN
                assert call(counts=(la.NQ, 0, nq, nk)) == ARG
            else:
                assert call(counts=(la.NQ + 2, la.NK)) == ALIGN
        after = la.everything()
        for n in o:
            assert torch.equal(after[n].buf, o[n].buf), f"a refused call wrote {n}"
