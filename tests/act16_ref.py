"""Host infrastructure of the 16-bit activation-map edge tests (tests/test_gpu_act16_edges.py, tests/test_cpu_act16_edges.py):
plain torch / numpy, no GPU in here.

- 16-bit maps: bits of a bf16 / fp16 map, the written mask of a 16-bit map that lies in a buffer sized for the fp32 map, and the
  check of such a buffer 16-bit element by 16-bit element.
- flush_f16: the inputs of the fp16-forward / bf16-backward rows (every value exact in fp16 AND bf16).
- The out-projection + LayerNorm cases of the issue's table: inputs, the float64 restatement of csn_outproj_ln_fwd_f32 /
  csn_outproj_ln_bwd_f32 with a DERIVED bound beside every value, the same arithmetic restated in float32 numpy, and the
  mutations (a point, a channel row, the last 8-byte unit of a row dropped) the bounds are held against.
- The float64 reference of csn_project_f32 writing one 16-bit map.

THE BOUNDS (first order in U = 2^-24; a sum of k terms is charged k U sum |terms|, which covers the k - 1 additions in ANY order and
the second-order rest; operands hold 16-bit values, so every product of a contraction is exact in fp32):
  fc      = sum_D w ctx                          D U A,              A = sum_D |w ctx|
  z       = fc keep / (1 - p) + x                ks (D + 3) U A keep + U |z|      (1 / (1 - p) in fp32: 2 U, the product: U)
  mean    = sum_c z / C                          (C + 2) U mean_c |z| + mean_c E(z)
  dlt     = z - mean                             E(z) + E(mean) + U |dlt|
  var     = sum_c dlt^2 / C + eps                (sum_c 2 |dlt| E(dlt) + (C + 1) U sum_c dlt^2) / C + 3 U var
  rstd    = 1 / sqrt(var)                        rstd (E(var) / (2 var) + 4 U)
  xhat    = dlt rstd                             E(dlt) rstd + |dlt| E(rstd) + U |xhat|
  sums    = sum_n xhat                           sum_n E(xhat) + NP U sum_n |xhat|
  gx      = scale dxhat + rows   (one fma)       U |gx|
  m1      = sum_c gx / C                         (C + 2) U mean_c |gx| + mean_c E(gx)
  m2      = sum_c gx xhat / C                    (C + 3) U mean_c |gx xhat| + mean_c E(gx) |xhat|
  t       = gx - m1 - xhat m2                    E(gx) + E(m1) + |xhat| E(m2) + U (|xhat m2| + |gx - m1| + |t|)
  dz_res  = rstd t                               rstd E(t) + U |dz_res|
  dz      = dz_res keep / (1 - p)                ks keep E(dz_res) + 3 U |dz|
  dctx    = sum_c w^T r16(dz)                    C U sum_c |w^T r16(dz)|          (r16: the mode's rounding of the staged operand)
  dwfc    = sum_{e,n} r16(dz) ctx                E NP U sum_{e,n} |r16(dz) ctx|
xhat and rstd of the backward are INPUTS (the forward's outputs as they are): no error of theirs enters its bounds.
(The kernels form z - sum / C and sq / C + eps with one fused multiply-add each: one rounding fewer than charged here.)"""
import numpy as np
import torch

from tests import attn_edge_ref as ar
from tests import dropout_ref as dr

U = 2.0 ** -24
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}         # unit roundoff of the 16-bit types (8 / 11 significant bits)
F16_MIN = 2.0 ** -14                                  # smallest normal fp16
FMT_OF = {1: "bf16", 2: "f16"}                        # csn_set_thread_act16(fmt & 3) -> the forward's 16-bit type
PAT_LO, PAT_HI = 0xA5A5 - 65536, 0x7FA5               # the two int16 halves of ar.CANARY32 (little endian: low half first)


# ---- 16-bit maps ------------------------------------------------------------------------------------------------------------
def dtype16(fmt):
    return torch.bfloat16 if fmt == "bf16" else torch.float16


def nan16(fmt):
    return ar.NAN_BF16 if fmt == "bf16" else ar.NAN_F16


def bits16(x, fmt):
    """fp32 tensor -> int16 bits of the value rounded once (nearest even) to bf16 / fp16"""
    return x.to(dtype16(fmt)).view(torch.int16)


def widen16(bits, fmt):
    """int16 bits -> the fp32 value they hold"""
    return bits.view(dtype16(fmt)).float()


def map_written(n_slots, slots, stride, D, ld, N, device="cpu"):
    """the element mask of maps [slot][D][ld] of slot stride `stride` elements: points < N of every row of every listed slot
    (tests/test_gpu_attn_edges.py _map_written, for any device)"""
    m = torch.zeros((n_slots, stride), dtype=torch.bool, device=device)
    for s in slots:
        m[s, :D * ld].view(D, ld)[:, :N] = True
    return m


def map_written16(n_slots, slots, stride, D, ld, N, device="cpu"):
    """the same map as ONE 16-bit plane inside the buffer of the fp32 map (n_slots * stride fp32 elements = twice as many 16-bit
    ones): strides and pitches count 16-bit elements with the same numbers, so the mask of the first n_slots * stride 16-bit
    elements is the fp32 map's and the second half of the buffer is never written.  Flat, 2 * n_slots * stride elements."""
    m = map_written(n_slots, slots, stride, D, ld, N, device).reshape(-1)
    return torch.cat((m, torch.zeros_like(m)))


def pattern16(n32, device="cpu"):
    """the int16 view of n32 fp32 elements that hold ar.CANARY32"""
    return torch.tensor([PAT_LO, PAT_HI], dtype=torch.int16, device=device).repeat(n32)


def touched16(body32, written16):
    """number of 16-bit elements outside `written16` (flat bool, 2 per int32 of body32) that no longer hold the canary pattern"""
    b = body32.contiguous().view(torch.int16)
    return int(((b != pattern16(body32.numel(), b.device)) & ~written16.reshape(-1)).sum())


def flush_f16(x):
    """|v| < 2^-14 -> 0: a bf16 value that survives is a NORMAL fp16 value (8 significant bits, |v| < 65504), so the map is exact
    in both 16-bit types and the fp16 -> bf16 conversion of the backward's staging is exact"""
    return torch.where(x.abs() < F16_MIN, torch.zeros_like(x), x)


def flushed_row_inputs(r):
    """ar.row_inputs of a mode-2 row with every map flushed"""
    return tuple(flush_f16(t) for t in ar.row_inputs(r))


# ---- out-projection + LayerNorm -----------------------------------------------------------------------------------------------
E_OUT, S_OUT, RES_INDEX = 3, 2, (1, 0, 1)
EPS_LN = 1e-6
# (C, D, NP, ld): the edge each shape is chosen for is named in the issue's table and in tests/test_gpu_act16_edges.py
OUTPROJ_SHAPES = [(32, 32, 4, 4), (32, 36, 60, 64), (64, 64, 124, 128), (96, 100, 132, 132), (128, 128, 68, 72),
                  (256, 256, 220, 224), (256, 256, 224, 224), (256, 64, 260, 264), (256, 192, 508, 512), (128, 256, 228, 228)]
OUTPROJ_DROPOUT = (1, 6, 8)                          # the second, seventh and ninth shape: p = 0.1, a seed with high bits
OUTPROJ_OUTPUTS_FWD = ("xhat", "rstd", "sums")
OUTPROJ_OUTPUTS_BWD = ("dz", "dz_res", "dctx", "dwfc")
SPIKE_X, SPIKE_G = 24.0, 16.0


def outproj_id(i):
    C, D, NP, ld = OUTPROJ_SHAPES[i]
    return f"C{C}-D{D}-NP{NP}-ld{ld}" + ("-p0.1" if i in OUTPROJ_DROPOUT else "")


def outproj_case(i, fmt, shape=None, n_evals=E_OUT, p=None, spike_x=SPIKE_X, spike_g=SPIKE_G, spike_w=None):
    """Inputs of shape i with 16-bit operands of type fmt: ctx (E, D, ld), w (C, D), dxhat (E, C, ld) hold 16-bit values, the
    residual x (S, C, ld), rows (E, C) and scale (E, C) full fp32; keep (E, C, NP) the fc dropout mask (all True without).
    Two points carry weight of their own, so that a sum over ~1500 points still shows ONE missing point at 10x its bound: the last
    point (NP - 1) and the first of the last 8-byte unit of a 16-bit row (NP - 4) have one residual channel of SPIKE_X (|xhat|
    there ~ sqrt(C) / 2), one ctx row and one gradient channel of SPIKE_G.
    For tests/outproj_edge_ref.py (the defaults are the cases above, bit for bit): fmt None leaves the operands full fp32 (no
    rounding, no flush); shape = (C, D, NP, ld) another shape than OUTPROJ_SHAPES[i] (i then only seeds the case); n_evals the
    case's own number of evaluations (residual slots (e + 1) % S_OUT); p its dropout probability; spike_x / spike_g its spikes;
    spike_w a third one: the weight that joins the last point's spiked ctx row to its spiked residual channel."""
    C, D, NP, ld = OUTPROJ_SHAPES[i] if shape is None else shape
    E = n_evals
    rng = np.random.default_rng(9100 + i)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    ctx, w, x = f(E, D, ld), f(C, D) / D ** 0.5, f(S_OUT, C, ld)
    dxhat, rows, scale = f(E, C, ld), 0.25 * f(E, C), f(E, C)
    for n, c, d in ((NP - 1, 5, D - 1), (NP - 4, 7, D - 2)):
        x[:, c, n] = spike_x
        ctx[:, d, n] = spike_g
        dxhat[:, c + 4, n] = spike_g
    if spike_w is not None:
        w[5, D - 1] = spike_w
    if fmt is not None:
        ctx, w, dxhat = (ar.round16(t, fmt) for t in (ctx, w, dxhat))
        ctx = flush_f16(ctx)                              # (a bf16 Ctx is then exact as the fp16 map of an fp16 forward too)
    if p is None:
        p = 0.1 if i in OUTPROJ_DROPOUT else 0.0
    seed = ar.HIGH_SEED + 31 * i
    keep = torch.from_numpy(dr.fc_mask(E, C, NP, seed, p, ld)) if p > 0 else torch.ones((E, C, NP), dtype=torch.bool)
    return dict(C=C, D=D, NP=NP, ld=ld, fmt=fmt, ctx=ctx, w=w, x=x, dxhat=dxhat, rows=rows, scale=scale, p=p, seed=seed, keep=keep,
                E=E, res_index=tuple((e + 1) % S_OUT for e in range(E)))


# backward forms: (name, n_dense, rows, scale / group)
OUTPROJ_FORMS = [("dense", E_OUT, False, False), ("rows-scale-group2", E_OUT - 1, True, True)]


def _ks(p):
    return 1.0 / (1.0 - p)


def outproj_fwd(c, n_keep=None, drop_row=False, prod_err=0.0):
    """float64 forward of a case: dict name -> (value, bound) for xhat (E, C, NP), rstd (E, NP), sums (E, C).
    Mutations: n_keep < NP computes the first n_keep points only (the others are zero in every map and enter no sum); drop_row
    leaves the last ctx row out of the contraction.
    prod_err: an extra error of the contraction, as a multiple of A = sum_D |w ctx| (operands that are not 16-bit values)."""
    C, D, NP = c["C"], c["D"], c["NP"]
    Dk = D - 1 if drop_row else D
    w, ctx = c["w"].double()[:, :Dk], c["ctx"].double()[:, :Dk, :NP]
    xr = c["x"].double()[list(c.get("res_index", RES_INDEX))][..., :NP]
    keep, ks = c["keep"].double(), _ks(c["p"])
    fc = torch.einsum("cd,edn->ecn", w, ctx)
    A = torch.einsum("cd,edn->ecn", w.abs(), ctx.abs())
    z = fc * keep * ks + xr
    Ez = U * (ks * (D + 3) * A * keep + z.abs())
    if prod_err:
        Ez = Ez + prod_err * ks * A * keep
    mean = z.mean(1, keepdim=True)
    Em = (C + 2) * U * z.abs().mean(1, keepdim=True) + Ez.mean(1, keepdim=True)
    dlt = z - mean
    Ed = Ez + Em + U * dlt.abs()
    sq = (dlt * dlt).sum(1)
    var = sq / C + EPS_LN
    Ev = ((2 * dlt.abs() * Ed).sum(1) + (C + 1) * U * sq) / C + 3 * U * var
    rstd = var ** -0.5
    Er = rstd * (0.5 * Ev / var + 4 * U)
    xhat = dlt * rstd[:, None]
    Ex = Ed * rstd[:, None] + dlt.abs() * Er[:, None] + U * xhat.abs()
    if n_keep is not None:
        xhat, rstd = xhat.clone(), rstd.clone()
        xhat[..., n_keep:] = 0
        rstd[..., n_keep:] = 0
    sums = xhat.sum(2)
    Es = Ex.sum(2) + NP * U * xhat.abs().sum(2)
    return {"xhat": (xhat, Ex), "rstd": (rstd, Er), "sums": (sums, Es)}


def outproj_gx(c, form):
    """the incoming gradient of a backward form, float64 (E, C, NP): scale[e] dxhat[e / group] on the dense evaluations + rows"""
    _, n_dense, use_rows, use_scale = form
    NP = c["NP"]
    dx = c["dxhat"].double()[..., :NP]
    gx = torch.zeros_like(dx)
    for e in range(n_dense):
        gx[e] = c["scale"].double()[e][:, None] * dx[e // 2] if use_scale else dx[e]
    if use_rows:
        gx = gx + c["rows"].double()[:, :, None]
    return gx


def outproj_ln_bwd(c, form, xhat, rstd, n_keep=None, drop_row=False):
    """float64 LayerNorm backward of a case from GIVEN xhat (E, C, NP) and rstd (E, NP): name -> (value, bound) for dz, dz_res.
    Mutations: the points from n_keep on are zero; drop_row leaves the last channel out of the two channel sums."""
    C, NP = c["C"], c["NP"]
    xhat, rstd = xhat.double(), rstd.double()[:, None]
    gx = outproj_gx(c, form)
    Eg = U * gx.abs()
    Ck = C - 1 if drop_row else C
    m1 = gx[:, :Ck].sum(1, keepdim=True) / C
    Em1 = (C + 2) * U * gx.abs().mean(1, keepdim=True) + Eg.mean(1, keepdim=True)
    pr = gx * xhat
    m2 = pr[:, :Ck].sum(1, keepdim=True) / C
    Em2 = (C + 3) * U * pr.abs().mean(1, keepdim=True) + (Eg * xhat.abs()).mean(1, keepdim=True)
    t = gx - m1 - xhat * m2
    Et = Eg + Em1 + xhat.abs() * Em2 + U * ((xhat * m2).abs() + (gx - m1).abs() + t.abs())
    dzr = rstd * t
    Er = rstd * Et + U * dzr.abs()
    keep, ks = c["keep"].double(), _ks(c["p"])
    dz = dzr * keep * ks
    Ez = ks * keep * Er + 3 * U * dz.abs()
    if n_keep is not None:
        dz, dzr = dz.clone(), dzr.clone()
        dz[..., n_keep:] = 0
        dzr[..., n_keep:] = 0
    return {"dz": (dz, Ez), "dz_res": (dzr, Er)}


def outproj_products(c, dz, ctx=None, n_keep=None, drop_row=False, round_dz=True, prod_err=(0.0, 0.0)):
    """float64 dctx = w^T r16(dz) (E, D, NP) and dwfc = sum_{e,n} r16(dz) ctx (C, D) from a GIVEN dz (E, C, NP), rounded to bf16 as
    the backward (math mode 2) stages it: name -> (value, bound).  ctx: another Ctx than the case's (the 16-bit map's values).
    Mutations: points from n_keep on enter no sum and are zero in dctx; drop_row leaves the last dz channel out of dctx and dwfc.
    round_dz False: dz enters the products as it is (math modes 0 and 1); prod_err: an extra error of the two contractions, as
    multiples of sum |w^T dz| and of sum |dz ctx|."""
    C, D, NP = c["C"], c["D"], c["NP"]
    dzb = ar.round16(dz.float(), "bf16").double() if round_dz else dz.double()
    if drop_row:
        dzb = dzb.clone()
        dzb[:, C - 1] = 0
    w = c["w"].double()
    cx = (c["ctx"] if ctx is None else ctx).double()[..., :NP]
    dctx = torch.einsum("cd,ecn->edn", w, dzb)
    Ac = torch.einsum("cd,ecn->edn", w.abs(), dzb.abs())
    Ec = C * U * Ac
    if prod_err[0]:
        Ec = Ec + prod_err[0] * Ac
    nk = NP if n_keep is None else n_keep
    if n_keep is not None:
        dctx = dctx.clone()
        dctx[..., n_keep:] = 0
    dw = torch.einsum("ecn,edn->cd", dzb[..., :nk], cx[..., :nk])
    Aw = torch.einsum("ecn,edn->cd", dzb.abs(), cx.abs())
    Ew = c.get("E", E_OUT) * NP * U * Aw
    if prod_err[1]:
        Ew = Ew + prod_err[1] * Aw
    return {"dctx": (dctx, Ec), "dwfc": (dw, Ew)}


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (nan in got: inf)"""
    d = (got.double().cpu() - ref.double().cpu()).abs() / bound.double().cpu().clamp_min(1e-300)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return d.max().item() if d.numel() else 0.0


# the same arithmetic in float32 numpy, every step rounded as the kernels round it (sums by numpy: pairwise, one of the orders)
def outproj_fwd_f32(c):
    C, NP = c["C"], c["NP"]
    f = np.float32
    w, ctx = c["w"].numpy(), c["ctx"].numpy()[..., :NP]
    xr = c["x"].numpy()[list(RES_INDEX)][..., :NP]
    keep = c["keep"].numpy()
    ks = f(1) / (f(1) - f(c["p"]))
    fc = np.stack([w @ ctx[e] for e in range(E_OUT)]).astype(f)
    z = np.where(keep, fc * ks, f(0)) + xr
    mean = z.sum(1, keepdims=True, dtype=f) * f(1.0 / C)
    dlt = z - mean
    sq = (dlt * dlt).sum(1, dtype=f)
    rstd = f(1) / np.sqrt(sq * f(1.0 / C) + f(EPS_LN))
    xhat = dlt * rstd[:, None]
    return {"xhat": xhat, "rstd": rstd, "sums": xhat.sum(2, dtype=f)}


def outproj_bwd_f32(c, form, xhat, rstd):
    """float32 backward from given fp32 xhat, rstd: dz, dz_res, then dctx and dwfc from bf16(dz)"""
    C, NP = c["C"], c["NP"]
    f = np.float32
    _, n_dense, use_rows, use_scale = form
    gx = outproj_gx(c, form).numpy().astype(f)             # one fma: the float64 value rounded once
    m1 =gx.sum(1, keepdims=True, dtype=f) / f(C)
    m2 = (gx * xhat).sum(1, keepdims=True, dtype=f) / f(C)
    dzr = rstd[:, None] * (gx - m1 - xhat * m2)
    ks = f(1) / (f(1) - f(c["p"]))
    dz = np.where(c["keep"].numpy(), dzr * ks, f(0)).astype(f)
    dzb = torch.from_numpy(dz).bfloat16().float().numpy()
    w, ctx = c["w"].numpy(), c["ctx"].numpy()[..., :NP]
    dctx = np.stack([w.T @ dzb[e] for e in range(E_OUT)]).astype(f)
    dw = sum(dzb[e] @ ctx[e].T for e in range(E_OUT)).astype(f)
    return {"dz": dz, "dz_res": dzr.astype(f), "dctx": dctx, "dwfc": dw}


# ---- csn_project_f32 writing one 16-bit map ---------------------------------------------------------------------------------------
PROJECT16_SHAPES = [(2, 40, 36, 60), (1, 256, 256, 228), (2, 96, 96, 260)]       # (S, R, C, NP)
PROJECT16_TEMPERATURE = 5.5                                                      # not a power of two


def project16_case(i, fmt):
    S, R, C, NP = PROJECT16_SHAPES[i]
    rng = np.random.default_rng(4400 + i)
    x = ar.round16(torch.from_numpy(rng.standard_normal((S, C, NP)).astype(np.float32)), fmt)
    w = ar.round16(torch.from_numpy((rng.standard_normal((R, C)) / C ** 0.5).astype(np.float32)), fmt)
    return dict(S=S, R=R, C=C, NP=NP, x=x, w=w, div_rows=(R // 2 + 3) // 4 * 4, temperature=PROJECT16_TEMPERATURE)


def project16_ref(c, fmt):
    """float64 out[s][r][n] = sum_c w x (/ temperature on rows < div_rows) and the bound of its ONE rounding to 16 bits after fp32
    accumulation: U16 |out| (the rounding; twice the fp16 subnormal step below the normal range) + the fp32 error of the value
    that is rounded, (C + 4) U sum |w x| / t (C products exact, the sum, a division or a reciprocal and a product), which may also
    move the value across a rounding boundary: it enters twice."""
    w, x = c["w"].double(), c["x"].double()
    out = torch.einsum("rc,scn->srn", w, x)
    A = torch.einsum("rc,scn->srn", w.abs(), x.abs())
    div = torch.ones(c["R"], dtype=torch.float64)
    div[:c["div_rows"]] = c["temperature"]
    out, A = out / div[None, :, None], A / div[None, :, None]
    bound = U16[fmt] * out.abs() + 2 * (c["C"] + 4) * U * A + (2.0 ** -24 if fmt == "f16" else 0.0)
    return out, bound
