"""csn_outproj_ln_fwd_f32 / csn_outproj_ln_bwd_f32 in math modes 0 (fp32) and 1 (bf16x3, the mode the step runs in) at the edges of
every kernel behind them, through the raw C ABI, against float64 within the bounds DERIVED in tests/outproj_edge_ref.py (held
sound and sharp on the CPU by tests/test_cpu_outproj_edges.py; none is tuned on a GPU).  Inputs hold NaN past their last point and
between slots, evaluation strides of Ctx and of the residual are padded by 16 (the xhat maps stay dense, as xhat_sum requires),
every output lies in a canary buffer.  Mode 1 with C = D = 256 runs every route of CSN_DEV_WX: forward 9 (the stream from 224
points on), 5 (256 x 256 tiles), 1; backward 9 (LayerNorm backward fused into the dCtx stream — it asks for ONE evaluation stride of
xhat and Ctx, so that route's Ctx and dCtx are dense), 1 (LayerNorm backward, then the dCtx stream), 0 (then the tiled GEMM).

The edge each shape is there for (oe.CASES; the ten of a16.OUTPROJ_SHAPES run in both modes):
  (32, 32, 4, 4) four points;  (32, 36, 60, 64) D % 32 == 4 in the small kernel's 32-wide k slab, pitch above the count;
  (64, 64, 124, 128) one short 128-point tile;  (96, 100, 132, 132) a second tile of 4 points;  (128, 128, 68, 72) the LayerNorm
  backward's group of 64 + 4;  (256, 256, 220, 224) the last size on the small kernel — in mode 1 the backward is the fused stream
  with a 28-point last chunk;  (256, 256, 224, 224) the first on the stream / the big tiles;  (256, 64, 260, 264) ragged second
  tile, dCtx on the 64-row tile;  (256, 192, 508, 512) the 256 x 256 tiles with the sums epilogue (D != 256), dCtx M = 192;
  (128, 256, 228, 228) small forward kernel, big-tile dCtx.
  Mode 1, C = D = 256: (4, 4) the fused backward on one 4-point chunk;  (36, 40) a chunk plus 4 points, pitch above the count;
  (252, 256) p = 0.1, a 28-point last chunk on the forward stream;  (260, 264) E = 40, p = 0.1: 360 chunks on 256 work-groups, runs
  that cross evaluations at a 4-point chunk, more than one slot of fused point sums per evaluation.

Measured on an MI355X, worst error / derived bound over the cases of a mode, every route (every case prints its figures):
  mode 0:  xhat 0.029  rstd 0.028  xhat_sum 0.008  dz 0.289  dz_res 0.272  dCtx 0.091  dW_fc 0.163
  mode 1:  xhat 0.044  rstd 0.009  xhat_sum 0.014  dz 0.285  dz_res 0.231  dCtx 0.165  dW_fc 0.325
  dctx_split: the high plane is bf16(dCtx) bit for bit, |hi + lo - dCtx| / (u^2 |dCtx|) = 0.499.
Every case held as the kernels stood: guards intact, masks exact, two calls the same bits, xhat / rstd the same bits with and
without the sums' workspace.  (The dCtx figures of the fused route and of the two-launch routes differ in the third digit: they
are different kernels.)"""
import pytest
import torch

from tests import act16_ref as a16
from tests import attn_edge_ref as ar
from tests import outproj_edge_ref as oe
from tests.test_gpu_act16_edges import _put32, _stream

pytestmark = pytest.mark.gpu

Canary = ar.Canary
K = range(len(oe.CASES))
_worst = {}


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    lib = L.lib()
    group = lib.csn_dev_get(L.DEV_LNB_GROUP)
    yield
    lib.csn_set_math_mode(1)
    lib.csn_dev_set(L.DEV_WX, L.DEV_WX_DEFAULT)
    lib.csn_dev_set(L.DEV_LNB_GROUP, group)


def _hold(mode, name, got, ref_bound, out):
    r = a16.ratio(got, *ref_bound)
    out[name] = max(out.get(name, 0.0), r)
    key = (mode, name.split(" (")[0])
    _worst[key] = max(_worst.get(key, 0.0), r)
    assert r <= 1.0, f"{name}: error / derived bound = {r:.3f}"


class _OutProj:
    """the buffers and calls of one case"""

    def __init__(self, L, c):
        self.L, self.lib, self.c = L, L.lib(), c
        C, D, NP, ld, E = (c[n] for n in ("C", "D", "NP", "ld", "E"))
        self.E = E
        self.es, self.cs, self.xs = C * ld, D * ld + 16, C * ld + 16
        self.w = c["w"].cuda()
        self.wt = c["w"].t().contiguous().cuda()
        self.x = _put32(c["x"], NP, self.xs)
        self.res = torch.tensor(c["res_index"], dtype=torch.int32, device="cuda")
        self.ctx = {self.cs: _put32(c["ctx"], NP, self.cs)}            # by evaluation stride
        self.dxhat = _put32(c["dxhat"], NP, self.es)
        self.rows, self.scale = c["rows"].cuda(), c["scale"].cuda()
        self.xhat_w = a16.map_written(E, range(E), self.es, C, ld, NP, "cuda")
        self.all = lambda n: torch.ones(n, dtype=torch.bool, device="cuda")

    def route(self, wx):
        if wx is not None:
            assert self.lib.csn_dev_set(self.L.DEV_WX, wx) >= 0

    def ctx_of(self, stride):
        if stride not in self.ctx:
            self.ctx[stride] = _put32(self.c["ctx"], self.c["NP"], stride)
        return self.ctx[stride]

    def forward(self, wx, with_ws):
        c, lib, E = self.c, self.lib, self.E
        C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
        xhat, rstd, sums = Canary(E * self.es), Canary(E * NP), Canary(E * C)
        ws_n = lib.csn_outproj_ln_workspace_floats(E, C, D, NP) if with_ws else 0
        assert not with_ws or ws_n >= E * ((NP + 255) // 256) * C
        ws = torch.full((max(ws_n, 4),), float("nan"), device="cuda")
        self.L.check(lib.csn_set_math_mode(c["mode"]))
        self.route(wx)
        self.L.check(lib.csn_outproj_ln_fwd_f32(self.ctx[self.cs].data_ptr(), self.cs, self.w.data_ptr(), self.x.data_ptr(), self.xs,
                                                self.res.data_ptr(), xhat.ptr, self.es, rstd.ptr, E, C, D, ld, NP, a16.EPS_LN,
                                                c["p"], c["seed"], sums.ptr, ws.data_ptr() if with_ws else None, ws_n, _stream()),
                     "csn_outproj_ln_fwd_f32")
        xhat.check(self.xhat_w, "xhat")
        rstd.check(self.all(rstd.n), "rstd")
        sums.check(self.all(sums.n), "xhat_sum")
        return xhat, rstd, sums

    def maps(self, cn, R, stride):
        c = self.c
        return cn.f32().view(self.E, stride)[:, :R * c["ld"]].view(self.E, R, c["ld"])[..., :c["NP"]]

    def backward(self, wx, cs, form, with_res, xhat, rstd, split=0):
        """cs: the evaluation stride of Ctx and dCtx of this call.  split: dCtx leaves as two bf16 planes [evaluation][2][D][ld]"""
        c, lib, E = self.c, self.lib, self.E
        C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
        _, n_dense, use_rows, use_scale = form
        dz = Canary(E * self.es)
        dzr = Canary(E * self.es) if with_res else None
        dctx, dw = Canary(E * cs), Canary(C * D)                         # (split: 2 E cs bf16 elements are E cs fp32 ones)
        ws_n = lib.csn_wgrad_workspace_floats(C, D, E, NP)
        ws = torch.full((ws_n,), float("nan"), device="cuda")
        self.L.check(lib.csn_set_math_mode(c["mode"]))
        self.route(wx)
        self.L.check(lib.csn_outproj_ln_bwd_f32(self.dxhat.data_ptr(), xhat.ptr, rstd.ptr, self.es, self.ctx_of(cs).data_ptr(), cs,
                                                self.wt.data_ptr(), dz.ptr, dzr.ptr if dzr else None, dctx.ptr, dw.ptr,
                                                ws.data_ptr(), ws_n, E, C, D, ld, NP, 0, c["p"], c["seed"], split, cs if split else 0,
                                                self.rows.data_ptr() if use_rows else None, n_dense,
                                                self.scale.data_ptr() if use_scale else None, 2 if use_scale else 1, _stream()),
                     "csn_outproj_ln_bwd_f32")
        dz.check(self.xhat_w, "dz")
        if with_res:
            dzr.check(self.xhat_w, "dz_res")
        if not split:
            dctx.check(a16.map_written(E, range(E), cs, D, ld, NP, "cuda"), "dctx")
        dw.check(self.all(dw.n), "dwfc")
        return dz, dzr, dctx, dw


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, what):
        assert (x is None and y is None) or torch.equal(x.buf, y.buf), f"{name}: two identical calls differ"


@pytest.mark.parametrize("k", K, ids=[oe.case_id(k) for k in K])
def test_outproj_ln_at_the_edges(L, k):
    c = oe.case(k)
    o = _OutProj(L, c)
    cd = oe.on(c, "cuda")                                                 # the float64 reference runs on the device
    mode, C, D, NP, E = (c[n] for n in ("mode", "C", "D", "NP", "E"))
    fwd_routes, bwd_routes = oe.routes(c)
    out = {}

    # ---- forward: every route, with and without the sums' workspace
    ref = oe.fwd(cd)
    first = None
    for wx in fwd_routes:
        tag = "" if wx is None else f" (wx {wx})"
        got = {}
        for with_ws in (True, False):
            xhat, rstd, sums = got[with_ws] = o.forward(wx, with_ws)
            _hold(mode, "xhat" + tag, o.maps(xhat, C, o.es), ref["xhat"], out)
            _hold(mode, "rstd" + tag, rstd.f32().view(E, NP), ref["rstd"], out)
            _hold(mode, "xhat_sum" + tag + ("" if with_ws else " (no workspace)"), sums.f32().view(E, C), ref["sums"], out)
        assert torch.equal(got[True][0].buf, got[False][0].buf) and torch.equal(got[True][1].buf, got[False][1].buf), \
            "xhat / rstd differ with the sums' workspace"
        if first is None:
            first = got[True]
            _same_bits(first, o.forward(wx, True), ("xhat", "rstd", "xhat_sum"))
    xhat, rstd, _ = first                                                 # the default route's own xhat and rstd feed the backward
    xh_in, rs_in = o.maps(xhat, C, o.es).double(), rstd.f32().view(E, NP).double()

    # ---- backward: every route, both forms, with and without dz_res
    keep = cd["keep"]
    lns = {form[0]: oe.ln_bwd(cd, form, xh_in, rs_in) for form in oe.forms(E)}
    for wx in bwd_routes:
        tag = "" if wx is None else f" (wx {wx})"
        cs = o.es if wx == 9 else o.cs                                     # the fused route takes one stride for xhat and Ctx
        for form in oe.forms(E):
            ln = lns[form[0]]
            nz = ln["dz"][0] != 0
            for with_res in (True, False):
                res = dz, dzr, dctx, dw = o.backward(wx, cs, form, with_res, xhat, rstd)
                dzv = o.maps(dz, C, o.es)
                assert bool((dzv[~keep] == 0).all()), "dz: a dropped element is not an exact zero"
                assert torch.equal((dzv == 0)[nz], ~keep[nz]), "dz: the zeros are not the host mask's"
                _hold(mode, "dz" + tag, dzv, ln["dz"], out)
                if with_res:
                    rv = o.maps(dzr, C, o.es)
                    assert not bool((rv == 0)[nz & ~keep].any()), "dz_res carries the mask"
                    _hold(mode, "dz_res" + tag, rv, ln["dz_res"], out)
                pr = oe.products(cd, dzv)                                 # of the dz the call wrote
                _hold(mode, "dctx" + tag, o.maps(dctx, D, cs), pr["dctx"], out)
                _hold(mode, "dwfc" + tag, dw.f32().view(C, D), pr["dwfc"], out)
                if with_res and form[0] == "dense":
                    _same_bits(res, o.backward(wx, cs, form, with_res, xhat, rstd), ("dz", "dz_res", "dctx", "dwfc"))
    print(f"[outproj-edge] {oe.case_id(k)}: error / bound " + " ".join(f"{n} {r:.3f}" for n, r in out.items()))
    print("[outproj-edge] worst so far " + " ".join(f"mode{m} {n} {r:.3f}" for (m, n), r in sorted(_worst.items())))


def test_dctx_as_two_bf16_planes(L):
    """dctx_split = 1 (math mode 1; include/csn_hip.h SPLIT TENSORS): dCtx leaves as [evaluation][2][D][ld] bf16 planes of plane
    stride ctx_eval_stride.  The high plane is bf16(dCtx) of the unsplit call bit for bit, hi + lo within u^2 |dCtx| of it (lo =
    bf16(dCtx - hi): |dCtx - hi - lo| <= u |dCtx - hi| <= u^2 |dCtx|), nothing is written outside the two planes, and every other
    output is the unsplit call's."""
    k = next(i for i, s in enumerate(oe.CASES) if s[:5] == (1, 128, 128, 68, 72))
    c = oe.case(k)
    o = _OutProj(L, c)
    C, D, NP, ld, E = (c[n] for n in ("C", "D", "NP", "ld", "E"))
    xhat, rstd, _ = o.forward(None, True)
    form = oe.forms(E)[0]
    dz0, dzr0, dctx0, dw0 = o.backward(None, o.cs, form, True, xhat, rstd)
    dz1, dzr1, dctx1, dw1 = o.backward(None, o.cs, form, True, xhat, rstd, split=1)
    for a, b, name in ((dz0, dz1, "dz"), (dzr0, dzr1, "dz_res"), (dw0, dw1, "dwfc")):
        assert torch.equal(a.buf, b.buf), f"{name} differs when dCtx is split"
    written = a16.map_written(2 * E, range(2 * E), o.cs, D, ld, NP, "cuda")             # 2 E planes of stride cs, 16-bit elements
    bad = a16.touched16(dctx1.body, written)
    assert bad == 0, f"{bad} 16-bit elements outside the two planes were written"
    assert bool((torch.cat((dctx1.buf[:ar.GUARD], dctx1.buf[ar.GUARD + dctx1.n:])) == ar.CANARY32).all()), "a guard was written"
    planes = dctx1.body.view(torch.int16).view(E, 2, o.cs)[..., :D * ld].view(E, 2, D, ld)[..., :NP]
    want = o.maps(dctx0, D, o.cs)
    assert torch.equal(planes[:, 0], a16.bits16(want, "bf16")), "the high plane is not bf16(dCtx)"
    hi, lo = a16.widen16(planes[:, 0].contiguous(), "bf16").double(), a16.widen16(planes[:, 1].contiguous(), "bf16").double()
    r = a16.ratio(hi + lo, want.double(), oe.U_BF16 ** 2 * want.double().abs())
    print(f"[outproj-edge] dctx_split: |hi + lo - dCtx| / (u^2 |dCtx|) = {r:.3f}")
    assert r <= 1.0
