"""Host reference of the out-projection + LayerNorm edge tests in math modes 0 (fp32) and 1 (bf16x3)
(tests/test_gpu_outproj_edges.py, tests/test_cpu_outproj_edges.py): plain torch / numpy, no GPU needed in here.  Built on
tests/act16_ref.py: the same float64 restatement of csn_outproj_ln_fwd_f32 / csn_outproj_ln_bwd_f32 with a derived bound beside
every value, the same spikes and mutations, with the degrees of freedom these modes need — operands that are full fp32 (nothing is
rounded before the call), the case's own number of evaluations, dz entering dCtx and dW_fc as it is, and a per-product error term.

THE PER-PRODUCT TERM.  act16_ref's bounds hold for operands that are 16-bit values: every product exact in fp32, a contraction of K
terms charged K U A with A = sum |a b| and U = 2^-24.  The LayerNorm arithmetic is fp32 in every mode and keeps its bounds; the three
contractions (W_fc Ctx, dCtx = W_fc^T dz, dW_fc = sum dz Ctx) get, on top of K U A:

  mode 0 (fp32 operands, fp32 products): every product is rounded once, |fl(a b) - a b| <= U |a b|:             + U A

  mode 1 (bf16x3).  split4 (csn_common.h) writes v = hi + lo + r with hi = bf16(v), lo = bf16(v - hi); with u = 2^-8 the unit
  roundoff of bf16 (8 significant bits, round to nearest):
      |v - hi| <= u |v|     and v - hi is exact in fp32 (the 16 low bits of a 24-bit significand)
      |r| = |(v - hi) - lo| <= u |v - hi| <= u^2 |v|,      |hi| <= (1 + u) |v|,      |lo| <= (1 + u) u |v|
  wx_mma (wx_common.h; the tiled kernels issue the same three matrix instructions) accumulates al bh + ah bl + ah bh in fp32.
  What it leaves out of a b = (ah + al + ra)(bh + bl + rb) is
      a b - (ah bh + ah bl + al bh) = al bl + ra b + (a - ra) rb
      |.| <= (u^2 (1 + u)^2 + u^2 + (1 + u^2) u^2) |a b| = u^2 (3 + 2 u + 2 u^2) |a b| <= 3 u^2 (1 + u) |a b|
  Each of the three products has two 8-bit significands: exact in fp32.  Their 3 K terms are summed in fp32, charged 3 K U times
      sum |terms| <= ((1 + u)^2 + 2 u (1 + u)^2) |a b| = (1 + u)^2 (1 + 2 u) |a b| <= (1 + 5 u) |a b|
  so the contraction's error is (3 u^2 (1 + u) + 3 K U (1 + 5 u)) A, of which K U A is charged already:
                                                                                      + (3 u^2 (1 + u) + (2 + 15 u) K U) A
  (3 u^2 = 4.6e-5: at K = 256 three times the fp32 accumulation, K U = 1.5e-5.)

K is D in the forward, C in dCtx, E NP in dW_fc.  dz is NOT rounded to bf16 before the two backward products in these modes.
No figure in here comes from a GPU run: tests/test_cpu_outproj_edges.py holds every bound SOUND against a float32 / bf16x3 numpy
restatement of the kernels' arithmetic and SHARP against the three mutations at 10x."""
import numpy as np
import torch

from tests import act16_ref as a16

U, U_BF16 = a16.U, a16.U16["bf16"]
S_OUT = a16.S_OUT

# (mode, C, D, NP, ld, E, p): the ten shapes of a16.OUTPROJ_SHAPES with their three dropout cases in both modes, then the stream
# kernels' own edges (math mode 1, C = D = 256, 32-point chunks, one run of chunks per work-group)
_TEN = [(m, *a16.OUTPROJ_SHAPES[i], a16.E_OUT, 0.1 if i in a16.OUTPROJ_DROPOUT else 0.0)
        for m in (0, 1) for i in range(len(a16.OUTPROJ_SHAPES))]
_STREAM = [(1, 256, 256, 4, 4, 3, 0.0),              # the fused backward on one 4-point chunk
           (1, 256, 256, 36, 40, 3, 0.0),            # a chunk plus 4 points, pitch above the count (in the backward too)
           (1, 256, 256, 252, 256, 3, 0.1),          # last chunk of 28 points on the forward stream
           (1, 256, 256, 260, 264, 40, 0.1)]         # 9 chunks x 40 evaluations: runs cross evaluations at a 4-point chunk
CASES = _TEN + _STREAM
# the index that seeds a case: the ten shapes keep their act16 seeds in both modes
SEED_INDEX = [i for _ in (0, 1) for i in range(len(a16.OUTPROJ_SHAPES))] + [10 + k for k in range(len(_STREAM))]
# spikes (residual, ctx / gradient, weight) of the cases where a mutation falls short of 10x under the wider mode-1 bound with
# act16's two: xhat_sum under the dropped ctx row came to 4.5 .. 9.3 x its bound, which grows with the 3 u^2 term of EVERY point
# while the dropped row weighs in the last point alone.  Raising the two spikes cannot mend it: with P = |xhat| of the spiked
# channel at the last point (what the dropped point costs) and R its change when the row goes (what the dropped row costs), a
# row that only adds to the channel leaves P + R <= sqrt(C), and the sum of 508 points' bounds asks for more than sqrt(C) / 2
# of each.  So the ctx spike grows to 256 and a third spike, the weight that joins it to the spiked channel, is -3 (forty times
# a typical weight): the row then FLIPS the channel, -15 with it, +12 without.
SPIKES = {k: (a16.SPIKE_X, 16 * a16.SPIKE_G, -3.0) for k in (15, 16, 18, 19)}


def case_id(k):
    m, C, D, NP, ld, E, p = CASES[k]
    return f"mode{m}-C{C}-D{D}-NP{NP}-ld{ld}" + (f"-E{E}" if E != a16.E_OUT else "") + (f"-p{p}" if p else "")


def case(k):
    """the inputs of CASES[k] (a16.outproj_case: full fp32 operands) + its math mode"""
    m, C, D, NP, ld, E, p = CASES[k]
    sx, sg, sw = SPIKES.get(k, (a16.SPIKE_X, a16.SPIKE_G, None))
    c = a16.outproj_case(SEED_INDEX[k], None, shape=(C, D, NP, ld), n_evals=E, p=p, spike_x=sx, spike_g=sg, spike_w=sw)
    c["mode"] = m
    return c


def on(c, device):
    """the case with its tensors on `device` (the float64 reference then runs there)"""
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def forms(E):
    """a16.OUTPROJ_FORMS for E evaluations: dense, and rows + scale + group 2 with n_dense = E - 1"""
    return [("dense", E, False, False), ("rows-scale-group2", E - 1, True, True)]


def prod_err(mode, K):
    """the per-product term of a contraction of K terms, as a multiple of A = sum |a b| (module docstring)"""
    if mode == 0:
        return U
    u = U_BF16
    return 3 * u * u * (1 + u) + (2 + 15 * u) * K * U


def fwd(c, **mut):
    return a16.outproj_fwd(c, prod_err=prod_err(c["mode"], c["D"]), **mut)


def ln_bwd(c, form, xhat, rstd, **mut):
    return a16.outproj_ln_bwd(c, form, xhat, rstd, **mut)


def products(c, dz, **mut):
    pe = (prod_err(c["mode"], c["C"]), prod_err(c["mode"], c["E"] * c["NP"]))
    return a16.outproj_products(c, dz, round_dz=False, prod_err=pe, **mut)


def mutations(c):
    NP = c["NP"]
    return {"point": dict(n_keep=NP - 1), "row": dict(drop_row=True), "unit": dict(n_keep=NP - 4)}


def dropped_fraction(c):
    return 1.0 - c["keep"].double().mean().item()


# ---- the kernels' arithmetic restated in float32 numpy ------------------------------------------------------------------------
def split(v):
    """split4<Bf16x3>: hi = bf16(v), lo = bf16(v - hi), as fp32 arrays"""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.numpy(), lo.numpy()


def matmul(mode, a, b):
    """a @ b as the mode forms it: fp32, or the three bf16 products (lo hi, hi lo, hi hi) accumulated in fp32"""
    if mode == 0:
        return (a @ b).astype(np.float32)
    ah, al = split(a)
    bh, bl = split(b)
    return ((al @ bh + ah @ bl) + ah @ bh).astype(np.float32)


def fwd_f32(c):
    C, NP, E, m = c["C"], c["NP"], c["E"], c["mode"]
    f = np.float32
    w, ctx = c["w"].numpy(), c["ctx"].numpy()[..., :NP]
    xr = c["x"].numpy()[list(c["res_index"])][..., :NP]
    ks = f(1) / (f(1) - f(c["p"]))
    fc = np.stack([matmul(m, w, ctx[e]) for e in range(E)])
    z = np.where(c["keep"].numpy(), fc * ks, f(0)) + xr
    mean = z.sum(1, keepdims=True, dtype=f) * f(1.0 / C)
    dlt = z - mean
    sq = (dlt * dlt).sum(1, dtype=f)
    rstd = f(1) / np.sqrt(sq * f(1.0 / C) + f(a16.EPS_LN))
    xhat = dlt * rstd[:, None]
    return {"xhat": xhat, "rstd": rstd, "sums": xhat.sum(2, dtype=f)}


def bwd_f32(c, form, xhat, rstd):
    """float32 backward from given fp32 xhat, rstd: dz, dz_res, then dctx and dwfc from dz as it is"""
    C, NP, E, m = c["C"], c["NP"], c["E"], c["mode"]
    f = np.float32
    gx = a16.outproj_gx(c, form).numpy().astype(f)             # one fma: the float64 value rounded once
    m1 = gx.sum(1, keepdims=True, dtype=f) / f(C)
    m2 = (gx * xhat).sum(1, keepdims=True, dtype=f) / f(C)
    dzr = (rstd[:, None] * (gx - m1 - xhat * m2)).astype(f)
    ks = f(1) / (f(1) - f(c["p"]))
    dz = np.where(c["keep"].numpy(), dzr * ks, f(0)).astype(f)
    w, ctx = c["w"].numpy(), c["ctx"].numpy()[..., :NP]
    dctx = np.stack([matmul(m, w.T, dz[e]) for e in range(E)])
    dw = matmul(m, np.concatenate(list(dz), 1), np.concatenate(list(ctx), 1).T)
    return {"dz": dz, "dz_res": dzr, "dctx": dctx, "dwfc": dw}


# ---- the routes of a case (csn_capi.hip, gemm_bf16x3.hip: CSN_DEV_WX) --------------------------------------------------------
def routes(c):
    """(forward, backward) values of CSN_DEV_WX a case runs under; None: the default route only.
    C = D = 256 in math mode 1 — forward 9 the stream (from 224 points on), 5 the 256 x 256 tiles, 1; backward 9 the fused
    LayerNorm backward + dCtx stream, 1 LayerNorm backward then the dCtx stream, 0 LayerNorm backward then the tiled GEMM."""
    if c["mode"] == 1 and c["C"] == 256 and c["D"] == 256:
        return (9, 5, 1), (9, 1, 0)
    return (None,), (None,)
