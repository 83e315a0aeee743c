"""The score-free backward of the cross-length and ragged attention (include/csn_hip.h (3d): csn_cross_attn_bwd_flash_f32,
csn_varlen_attn_bwd_flash_f32) at every edge, through the raw C ABI, against the float64 reference of tests/cross_attn_ref.py:
every math-mode-1 row of the kept-scores sweep (tests/test_gpu_cross_attn_edges.py) at d_head <= 128 — 1 to 1301 keys, counts
that are no multiples of 4, a partial last query tile, the mask pitch max(n_queries, score_pitch), dropout, high seeds, ragged
batches.  The forward runs with scores = NULL; the padding of every input map holds finite sentinels, every output lies in a
NaN-pattern buffer with guards.

Allowances: the kept-scores sweep's own rule — BOUNDS[1] = (2e-4, 2e-4) of tests/attn_edge_ref.py, and for an evaluation with
more than 512 keys max(BOUNDS, 4 x err32), err32 = the distance from float64 of the same formula in torch float32 on the CPU."""
import pytest
import torch

from tests import attn_edge_ref as ar
from tests import cross_attn_ref as cr
from tests.test_gpu_cross_attn_edges import Launch

pytestmark = pytest.mark.gpu

ARG = -1
flash_row = lambda r: r["mode"] == 1 and r["d"] <= 128
CROSS = [r for r in cr.cross_rows() if flash_row(r)]
VARLEN = [r for r in cr.varlen_rows() if flash_row(r)]
OUTS = ("delta", "dq", "dk", "dv")


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


class FlashLaunch(Launch):
    """a row's inputs (tests/test_gpu_cross_attn_edges.py::Launch) with the score-free backward beside the kept-scores one"""

    def flash_rc(self, ctx_in, lse_in, delta, dq, dk, dv, **over):
        r = self.r
        a = dict(d=r["d"], Tp=r["Tp"], ld_q=r["ld_q"], ld_kv=r["ld_kv"], counts=self.counts())
        a.update(over)
        fn = self.lib.csn_varlen_attn_bwd_flash_f32 if self.varlen else self.lib.csn_cross_attn_bwd_flash_f32
        return fn(self.dd.data_ptr(), ctx_in.data_ptr(), r["q_stride"], self.qd.data_ptr(), self.kd.data_ptr(), self.vd.data_ptr(),
                  r["q_stride"], r["kv_stride"], a["ld_q"], a["ld_kv"], lse_in.data_ptr(), delta.ptr, dq.ptr, dk.ptr, dv.ptr,
                  r["q_stride"], r["kv_stride"], r["E"], r["H"], a["d"], *a["counts"], a["Tp"], r["p"], r["seed"], _stream())

    def outputs(self):
        r = self.r
        return dict(delta=ar.Canary(r["E"] * r["H"] * self.NQ), dq=ar.Canary(r["E"] * r["q_stride"]),
                    dk=ar.Canary(r["E"] * r["kv_stride"]), dv=ar.Canary(r["E"] * r["kv_stride"]))

    def flash(self, ctx_in, lse_in):
        out = self.outputs()
        self.L.check(self.flash_rc(ctx_in, lse_in, out["delta"], out["dq"], out["dk"], out["dv"]), "score-free backward")
        return out

    def score_free(self):
        """the flow: forward with scores = NULL, finite padding, score-free backward"""
        ctx, lse, _ = self.fwd(scores=False)
        return self.flash(*self.clean_inputs(ctx, lse))


def _reference(la):
    r = la.r
    E, H, d = r["E"], r["H"], r["d"]
    f64 = lambda t: t.double().view(E, H, d, -1).cuda()
    q, k, v, dctx = f64(la.q), f64(la.k), f64(la.v), f64(la.dctx)
    keep = cr.row_keep(r)
    ref = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep.cuda() if keep is not None else None, r["p"])
    cond = cr.row_condition(r, ref, q, k, v, dctx, keep)
    assert max(cond.values()) <= cr.COND_LIMIT, f"ill-conditioned draw (tests/cross_attn_ref.py REDRAW): {cond}"
    need32 = [r["nk"][e] > 512 for e in range(E)]
    ref32 = None
    if any(need32):
        c32 = lambda t: t.float().view(E, H, d, -1)
        ref32 = cr.cross_attention_ref(c32(la.q), c32(la.k), c32(la.v), c32(la.dctx), r["nq"], r["nk"], keep, r["p"], dtype=torch.float32)
    return (q, k, v, dctx), ref, ref32, need32


def _views(la, g, e):
    return dict(delta=la.stat(g["delta"], e), dq=la.q_map(g["dq"], e), dk=la.kv_map(g["dk"], e), dv=la.kv_map(g["dv"], e))


def _check_values(la, g, inputs, ref, ref32, need32, tag):
    """every output of every evaluation against float64 under the sweep's rule; returns {name: worst error / allowance}"""
    r = la.r
    q, k, v, dctx = inputs
    bound = ar.BOUNDS[1][1]
    worst, long_rows = {}, []
    for e in range(r["E"]):
        for name, got in _views(la, g, e).items():
            want = ref[e][name]
            scale = None
            if r["nk"][e] == 1 and name in ("dq", "dk"):                       # the reference is exactly zero: the natural scale
                assert float(want.abs().max()) == 0.0
                scale = cr.zero_scales(q[e], k[e], v[e], dctx[e], r["nq"][e], 1)[name]
            err = cr.eval_err(got, want, scale)
            allow = bound
            if need32[e]:
                e32 = cr.eval_err(ref32[e][name].cuda(), want, scale)
                allow = max(bound, 4 * e32)
                long_rows.append(f"{name} e{e} err32 {e32:.1e} kernel {err:.1e}")
            worst[name] = max(worst.get(name, 0.0), err / allow)
            assert err < allow, f"{tag} {name}, evaluation {e} ({r['nq'][e]} x {r['nk'][e]}): error {err:.3e} >= {allow:.2e}"
    print(f"[cross-flash] {cr.row_id(r)} {tag}: worst error / allowance " + " ".join(f"{n} {w:.2f}" for n, w in worst.items()))
    if long_rows:
        print(f"[cross-flash long] {cr.row_id(r)} {tag}: " + "; ".join(long_rows))
    return worst


def _check_row(L, r):
    L.check(L.lib().csn_set_math_mode(1))
    la = FlashLaunch(L, r)
    inputs, ref, ref32, need32 = _reference(la)
    ctx, lse, _ = la.fwd(scores=False)
    ctx_in, lse_in = la.clean_inputs(ctx, lse)
    g = la.flash(ctx_in, lse_in)
    # canaries: guards intact, everything outside the written regions of (3b) / (3c) keeps the pattern, the rest is written
    g["delta"].check(la.w_stat, "delta")
    g["dq"].check(la.w_q, "dq")
    g["dk"].check(la.w_kv, "dk")
    g["dv"].check(la.w_kv, "dv")
    for e in range(r["E"]):
        nk, nk4 = r["nk"][e], ar.ceil_to(r["nk"][e], 4)
        for n in ("dk", "dv"):
            assert bool((la.kv_map(g[n], e, nk4)[..., nk:] == 0).all()), f"{n}: the columns nk .. round-up-4(nk) are not exact zeros"
    _check_values(la, g, inputs, ref, ref32, need32, "score-free")
    g2 = la.flash(ctx_in, lse_in)
    for n in g:
        assert torch.equal(g2[n].buf, g[n].buf), f"score-free backward not repeatable: {n}"


@pytest.mark.parametrize("r", CROSS, ids=[cr.row_id(r) for r in CROSS])
def test_cross_score_free_edges(L, r):
    _check_row(L, r)


@pytest.mark.parametrize("r", VARLEN, ids=[cr.row_id(r) for r in VARLEN])
def test_varlen_score_free_edges(L, r):
    _check_row(L, r)


def _without_zero_signs(la, o):
    """the output buffers as bits, with -0 turned into +0 in the columns nk .. round-up-4(nk) of dk / dv (exact zeros whose
    sign may follow the padding; asserted to be zeros by the sweep above).  Every other bit must be identical."""
    r, G = la.r, ar.GUARD
    out = {n: c.buf.clone() for n, c in o.items()}
    D = r["H"] * r["d"]
    for n in ("dk", "dv"):
        body = out[n][G:G + r["E"] * r["kv_stride"]].view(r["E"], r["kv_stride"])
        for e in range(r["E"]):
            nk = r["nk"][e]
            x = body[e, :D * r["ld_kv"]].view(D, r["ld_kv"])[:, nk:ar.ceil_to(nk, 4)]
            x[x == -2 ** 31] = 0
    return out


RESENTINEL = [r for r in cr.resentinel_rows() if flash_row(r)]


@pytest.mark.parametrize("r", RESENTINEL, ids=[cr.row_id(r) for r in RESENTINEL])
def test_padding_is_not_read_as_data(L, r):
    """the same row with other sentinel values in every padding element of q, k, v, dctx, ctx, lse: every output bit-identical"""
    L.check(L.lib().csn_set_math_mode(1))
    la, lb = FlashLaunch(L, r, 0), FlashLaunch(L, r, 1)
    assert not torch.equal(la.kd, lb.kd) and not torch.equal(la.vd, lb.vd)
    a, b = _without_zero_signs(la, la.score_free()), _without_zero_signs(lb, lb.score_free())
    differ = [n for n in a if not torch.equal(a[n], b[n])]
    assert not differ, f"{differ} depend on the padding of the input maps"


def _one_row_per_width():
    """per head width one (3b) row with dropout and keys that are no multiple of 4 beyond one tile, and one ragged row"""
    out = []
    for d in (32, 64, 96, 128):
        c = [r for r in CROSS if r["d"] == d and r["p"] > 0 and r["nk"][0] > 32 and r["nk"][0] % 4]
        out.append(c[len(c) // 2])
        out.append([r for r in VARLEN if r["d"] == d][0])
    return out


BOTH = _one_row_per_width()


@pytest.mark.parametrize("r", BOTH, ids=[cr.row_id(r) for r in BOTH])
def test_both_flows_on_the_same_inputs(L, r):
    """The kept-scores backward and the score-free one on the same forward: no tolerance between the two — each lies within
    the sweep's rule of float64 — and their mutual distance is printed."""
    L.check(L.lib().csn_set_math_mode(1))
    la = FlashLaunch(L, r)
    inputs, ref, ref32, need32 = _reference(la)
    ctx, lse, sc = la.fwd()
    ctx_in, lse_in = la.clean_inputs(ctx, lse)
    kept = la.bwd(ctx_in, lse_in, sc)
    free = la.flash(ctx_in, lse_in)
    _check_values(la, kept, inputs, ref, ref32, need32, "kept scores")
    _check_values(la, free, inputs, ref, ref32, need32, "score-free")
    dist = {}
    for e in range(r["E"]):
        a, b = _views(la, kept, e), _views(la, free, e)
        for n in OUTS:
            den = float(ref[e][n].abs().max())
            if den > 0:
                dist[n] = max(dist.get(n, 0.0), float((a[n].double() - b[n].double()).abs().max()) / den)
    print(f"[cross-flash flows] {cr.row_id(r)}: kept vs score-free, max |a - b| / max |ref| " + " ".join(f"{n} {x:.1e}" for n, x in dist.items()))


OTHER = [r for r in cr.other_mode_rows() if flash_row(r)]


@pytest.mark.parametrize("r", OTHER, ids=[cr.row_id(r) for r in OTHER])
def test_modes_2_and_3_run_as_mode_1(L, r):
    """Math modes 2 and 3 run the score-free backward as mode 1, bit for bit, and leave the process mode and the calling
    thread's override as they were, also when the call returns an error."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    la = FlashLaunch(L, r)
    ctx, lse, _ = la.fwd(scores=False)
    ctx_in, lse_in = la.clean_inputs(ctx, lse)
    want = la.flash(ctx_in, lse_in)
    for mode, per_thread in ((2, False), (3, False), (2, True), (3, True)):
        if per_thread:
            L.check(lib.csn_set_math_mode(0))
            L.check(lib.csn_set_thread_math_mode(mode))
        else:
            L.check(lib.csn_set_thread_math_mode(-1))
            L.check(lib.csn_set_math_mode(mode))
        state = (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode())
        assert lib.csn_cross_attn_flash_available(r["d"]) == 1
        got = la.flash(ctx_in, lse_in)
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state, "a call changed the math mode"
        for n in want:
            assert torch.equal(got[n].buf, want[n].buf), f"mode {mode}: {n} differs from the mode-1 call"
        assert la.flash_rc(ctx_in, lse_in, got["delta"], got["dq"], got["dk"], got["dv"], d=40) == -5
        assert la.flash_rc(ctx_in, lse_in, got["delta"], got["dq"], got["dk"], got["dv"], d=256) == ARG
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state, "a failed call changed the math mode"
        for n in want:
            assert torch.equal(got[n].buf, want[n].buf), f"a refused call wrote {n}"


def test_mode_0_and_d256_are_refused(L):
    """no score-free flow in exact fp32 or at d_head = 256: CSN_E_ARG before any launch, the math mode left alone"""
    lib = L.lib()
    for r in (CROSS[10], VARLEN[0]):
        L.check(lib.csn_set_thread_math_mode(-1))
        L.check(lib.csn_set_math_mode(1))
        la = FlashLaunch(L, r)
        ctx, lse, _ = la.fwd(scores=False)
        ctx_in, lse_in = la.clean_inputs(ctx, lse)
        want = la.flash(ctx_in, lse_in)
        got = la.outputs()
        blank = {n: c.buf.clone() for n, c in got.items()}
        for mode, d, per_thread in ((1, 256, False), (0, r["d"], False), (0, r["d"], True), (0, 256, False)):
            if per_thread:
                L.check(lib.csn_set_math_mode(1))
                L.check(lib.csn_set_thread_math_mode(mode))
            else:
                L.check(lib.csn_set_thread_math_mode(-1))
                L.check(lib.csn_set_math_mode(mode))
            state = (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode())
            assert lib.csn_cross_attn_flash_available(d) == 0
            assert la.flash_rc(ctx_in, lse_in, got["delta"], got["dq"], got["dk"], got["dv"], d=d) == ARG
            assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state
            torch.cuda.synchronize()
            for n in got:
                assert torch.equal(got[n].buf, blank[n]), f"a refused call wrote {n}"
        L.check(lib.csn_set_thread_math_mode(-1))
        L.check(lib.csn_set_math_mode(1))
        again = la.flash(ctx_in, lse_in)
        for n in want:
            assert torch.equal(again[n].buf, want[n].buf)
