"""Host infrastructure of the attention edge sweep (tests/test_gpu_attn_edges.py, tests/test_cpu_attn_edges.py): plain
torch / numpy, like tests/dropout_ref.py.

- pack_tile_planes: the K / V tile planes of include/csn_hip.h (TILE PLANES), written from the contract: per row and block
  16 tiles of [hi 32 | lo 32] bf16 (math mode 1) or of [32] bf16 / fp16 (modes 2 / 3); the padding keys of a block's last
  32-key tile are zero and every tile past it — "never read" — is filled with NaN.
- attention_core: float64 autograd of softmax(Qs K^T) -> dropout -> @ V of one rectangular problem — the one implementation of
  the arithmetic, shared with the cross-length sweep (tests/cross_attn_ref.py).
- block_attention_ref: the same per (evaluation, head, block), short last block and keep mask included; returns ctx, lse, S,
  P_drop, dS, dQ, dK, dV.
- probe_inputs: queries / keys / values whose probe rows turn a one-key error of a kernel into an O(1) error.
- Canary: an output buffer of the GPU sweeps, filled with a NaN pattern and guarded on both sides.
- The row table of the sweep and the csn_attn_bwd_grouping rules restated as data.
"""
import math

import numpy as np
import torch

from tests import dropout_ref as dr

KT = 32                       # keys per tile
BLOCK_PITCH = 512             # 16-bit elements of one block of one plane (16 tiles of 32 keys)
NAN_BF16 = 0x7FA5             # NaN in bf16 (exponent all ones, mantissa 0x25)
NAN_F16 = 0x7E5A              # NaN in fp16 (exponent all ones, mantissa 0x25a)
CANARY32 = 0x7FA5A5A5         # NaN as fp32: the pattern every output buffer is filled with


def ceil_to(x, m):
    return (x + m - 1) // m * m


def block_lengths(T, nb, T_last=None):
    """Points of every block: nb - 1 full blocks and a last one of T_last points (None: full)."""
    return [T] * (nb - 1) + [T if T_last is None else T_last]


def n_points(T, nb, T_last=None):
    return sum(block_lengths(T, nb, T_last))


# ---- output buffers ------------------------------------------------------------------------------------------------------
GUARD = 64                     # int32 guard elements before and after every output


class Canary:
    """n fp32 elements inside a buffer of the NaN pattern with guards on both sides; compared as integers"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), CANARY32, dtype=torch.int32, device="cuda")

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.body.data_ptr()

    def f32(self):
        return self.body.view(torch.float32)

    def clone(self):
        c = Canary(self.n)
        c.buf.copy_(self.buf)
        return c

    def check(self, written, what):
        """guards intact; every element outside `written` (bool, n elements) still holds the pattern"""
        g = torch.cat((self.buf[:GUARD], self.buf[GUARD + self.n:]))
        assert bool((g == CANARY32).all()), f"{what}: a guard was written"
        untouched = self.body[~written.reshape(-1)]
        bad = int((untouched != CANARY32).sum())
        assert bad == 0, f"{what}: {bad} elements outside the contract's region were written"


# ---- tile planes ---------------------------------------------------------------------------------------------------------
def _bits16(x, fmt):
    """fp32 tensor -> int16 bits of bf16 / fp16"""
    return (x.bfloat16() if fmt == "bf16" else x.half()).view(torch.int16)


def pack_tile_planes(x, T, nb, npl, fmt="bf16", T_last=None):
    """fp32 (S, R, >= n_points) channel-major maps -> int16 tile planes (S, R, nb * 512 * npl).
    npl = 2 (math mode 1): per block 16 tiles of [hi: 32 keys | lo: 32 keys], hi = bf16(x), lo = bf16(x - hi).
    npl = 1 (modes 2 / 3): 16 tiles of [32 keys] of bf16 (fmt 'bf16') or fp16 (fmt 'f16').
    Keys of block b are x[..., b T : b T + T_b]; keys T_b .. round-up-32(T_b) are zero; the tiles past are NaN."""
    assert npl in (1, 2) and (npl == 1 or fmt == "bf16")
    S, R = x.shape[:2]
    nan = NAN_BF16 if fmt == "bf16" else NAN_F16
    out = torch.full((S, R, nb, 16, npl, KT), nan - 65536 if nan > 32767 else nan, dtype=torch.int16, device=x.device)
    for b, Tb in enumerate(block_lengths(T, nb, T_last)):
        nt = ceil_to(Tb, KT) // KT
        blk = torch.zeros((S, R, nt * KT), dtype=torch.float32, device=x.device)
        blk[..., :Tb] = x[..., b * T: b * T + Tb].float()
        blk = blk.view(S, R, nt, KT)
        hi = _bits16(blk, fmt)
        out[:, :, b, :nt, 0] = hi
        if npl == 2:
            out[:, :, b, :nt, 1] = _bits16(blk - hi.view(torch.bfloat16).float(), fmt)
    return out.reshape(S, R, nb * BLOCK_PITCH * npl).contiguous()


def unpack_tile_planes(planes, nb, npl, fmt="bf16"):
    """int16 tile planes -> fp32 values (S, R, nb, 512 keys) (hi + lo in mode 1): NaN where a tile holds NaN."""
    S, R = planes.shape[:2]
    v = planes.reshape(S, R, nb, 16, npl, KT)
    f = (lambda t: t.view(torch.bfloat16).float()) if fmt == "bf16" else (lambda t: t.view(torch.float16).float())
    val = f(v[:, :, :, :, 0].contiguous())
    if npl == 2:
        val = val + f(v[:, :, :, :, 1].contiguous())
    return val.reshape(S, R, nb, 16 * KT)


def round16(x, fmt):
    """the value of x rounded once to the mode's 16 bits (the operands of the one-plane modes)"""
    return (x.bfloat16() if fmt == "bf16" else x.half()).float() if fmt else x


# ---- dropout masks of the block attention ---------------------------------------------------------------------------------
def block_keep(E, H, T, nb, Tp, seed, p, extra_keys=0):
    """keep[e][h][blk][query][key] (bool, torch) of the scores geometry [E][H][nb][T][Tp]: dropout_ref.attention_mask of the
    FULL block (its pair index key/2 * max(Tp, T) + query on score_pitch); a short last block uses the full block's mask cut
    to its first T_last keys and queries (the kernels index the mask with the block's full query count — attn_f32.hip
    `mp = max(Tq, Tp)` with Tq = block).  extra_keys > 0 also draws the keys T .. T + extra_keys - 1 of the same pitch (the
    shifted-mask negative control)."""
    if p <= 0:
        return None
    m = dr.attention_mask(E, H, nb, T + extra_keys, Tp, seed, p, Tq=T)      # [e][h][blk][key][query]
    return torch.from_numpy(np.ascontiguousarray(m.transpose(0, 1, 2, 4, 3)))   # -> [query][key]


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def attention_core(q, k, v, dO, keep=None, scale=1.0, extra_k=None, extra_v=None, grads=True, dtype=torch.float64):
    """The arithmetic of every reference of the sweeps, once: autograd of softmax(Qs K^T) -> dropout -> @ V for a batch of
    rectangular problems.  q, dO: (..., d, nq); k, v: (..., d, nk); keep: (..., nq, nk) bool or None, scale = 1 / (1 - p);
    extra_k / extra_v: (..., d, n) keys let in after the real ones, always kept (the padding control).  Returns in `dtype`
    ctx, dq (..., d, nq); dk, dv (..., d, nk) — the real keys only; lse, delta (..., nq); S, P (after dropout), dS
    (..., nq, nk + n) [query][key].  grads = False: the forward quantities alone."""
    dev = q.device
    qb = q.to(dtype).detach().requires_grad_(grads)
    kb = k.to(dtype).detach().requires_grad_(grads)
    vb = v.to(dtype).detach().requires_grad_(grads)
    kk, vv = kb, vb
    n_extra = 0
    if extra_k is not None:
        n_extra = extra_k.shape[-1]
        kk, vv = torch.cat((kb, extra_k.to(dtype)), -1), torch.cat((vb, extra_v.to(dtype)), -1)
    s = qb.transpose(-1, -2) @ kk                                       # [query][key]
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        m = keep.to(dev).to(dtype)
        if n_extra:
            m = torch.cat((m, torch.ones(m.shape[:-1] + (n_extra,), dtype=dtype, device=dev)), -1)
        pr = pr * m * scale
    ctx = (pr @ vv.transpose(-1, -2)).transpose(-1, -2)                 # (..., d, nq)
    out = {"ctx": ctx.detach(), "lse": torch.logsumexp(s.detach(), dim=-1), "S": s.detach(), "P": pr.detach()}
    if grads:
        s.retain_grad()
        ctx.backward(dO.to(dtype))
        out.update(dq=qb.grad, dk=kb.grad, dv=vb.grad, dS=s.grad, delta=(dO.to(dtype) * ctx.detach()).sum(-2))
    return out


def block_attention_ref(q, k, v, dctx, T, nb, T_last=None, keep=None, p=0.0, drop_last_key=False, pad_keys=0):
    """float64 autograd of block attention.  q, k, v, dctx: (E, H, d, >= n_points) per EVALUATION (slots already gathered).
    keep: [E][H][nb][T][>= T] bool ([query][key]) or None.  Negative controls: drop_last_key removes key T_b - 1 of every
    block; pad_keys = n lets n zero keys (score 0, value 0) into every block, kept by the mask.
    Returns a dict of float64 tensors:
      ctx, dq, dk, dv (E, H, d, N): zero past the last point;  lse (E, H, nb T): NaN past the last point;
      S, P (after dropout), dS (E, H, nb, T, T) [query][key]: zero outside a block's T_b x T_b square."""
    E, H, d, N = q.shape
    dev = q.device
    scale = 1.0 / (1.0 - p) if keep is not None else 1.0
    out = {n: torch.zeros((E, H, d, N), dtype=torch.float64, device=dev) for n in ("ctx", "dq", "dk", "dv")}
    out["lse"] = torch.full((E, H, nb * T), float("nan"), dtype=torch.float64, device=dev)
    for n in ("S", "P", "dS"):
        out[n] = torch.zeros((E, H, nb, T, T), dtype=torch.float64, device=dev)
    for b, Tb in enumerate(block_lengths(T, nb, T_last)):
        c0 = b * T
        nk = Tb - 1 if drop_last_key else Tb
        z = torch.zeros((E, H, d, pad_keys), dtype=torch.float64, device=dev) if pad_keys else None
        r = attention_core(q[..., c0:c0 + Tb], k[..., c0:c0 + nk], v[..., c0:c0 + nk], dctx[..., c0:c0 + Tb],
                           keep[:, :, b, :Tb, :nk] if keep is not None else None, scale, z, z)
        out["ctx"][..., c0:c0 + Tb] = r["ctx"]
        out["dq"][..., c0:c0 + Tb] = r["dq"]
        out["dk"][..., c0:c0 + nk] = r["dk"]
        out["dv"][..., c0:c0 + nk] = r["dv"]
        out["lse"][..., c0:c0 + Tb] = r["lse"]
        out["S"][:, :, b, :Tb, :nk] = r["S"][..., :nk]
        out["P"][:, :, b, :Tb, :nk] = r["P"][..., :nk]
        out["dS"][:, :, b, :Tb, :nk] = r["dS"][..., :nk]
    return out


def per_block_err(got, ref, T, nb, T_last=None):
    """max over (evaluation, head, block) of max|got - ref| / max|ref| inside the block — so that an error confined to the short
    last block is not diluted by the others.  Maps (E, H, d, N) are cut along the points; score tensors (E, H, nb, T, T) and
    statistics (E, H, nb T) per block.  NaN in got (an element never written, or a NaN read) counts as an infinite error."""
    got, ref = got.double(), ref.double().to(got.device)
    worst = 0.0
    for b, Tb in enumerate(block_lengths(T, nb, T_last)):
        if got.dim() == 5:
            g, r = got[:, :, b, :Tb, :Tb], ref[:, :, b, :Tb, :Tb]
            g, r = g.reshape(g.shape[0], g.shape[1], -1), r.reshape(r.shape[0], r.shape[1], -1)
        elif got.dim() == 4:
            g, r = got[..., b * T: b * T + Tb], ref[..., b * T: b * T + Tb]
            g, r = g.reshape(g.shape[0], g.shape[1], -1), r.reshape(r.shape[0], r.shape[1], -1)
        else:
            g, r = got[..., b * T: b * T + Tb], ref[..., b * T: b * T + Tb]
        diff = (g - r).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        e = diff.amax(-1) / r.abs().amax(-1).clamp_min(1e-30)
        worst = max(worst, e.max().item())
    return worst


# ---- probe inputs ---------------------------------------------------------------------------------------------------------
SPIKE = 12.0      # score of a spiked key for its probe queries: e^12 / 512 ~ 300, the key takes > 99.6 % of the row
ROLE_NORMAL, ROLE_LAST, ROLE_TILE, ROLE_NEG, ROLE_FIRST = 0, 1, 2, 3, 4
# probe channels of every head: a query of role r puts +-SPIKE on channel r - 1, its target key(s) carry 1 there
CH_LAST, CH_TILE, CH_NEG, CH_FIRST = 0, 1, 2, 3
# the keys' entry on CH_NEG: small, because there dQ = sum_j dS_j k_j = 0 exactly and the computed value is rounding alone
NEG_K = 0.25
OFF = list(range(4, 12))      # value-offset channels of every head (probe_inputs)


def probe_keys(Tb):
    """(last valid key, first key of the last (partial) 32-key tile) of a block of T_b keys"""
    return Tb - 1, (Tb - 1) // KT * KT


def query_roles(Tb):
    """role of every query of a block of T_b points: spike on the last valid key (ROLE_LAST; the last query row always),
    spike on the first key of the last tile (ROLE_TILE), every real key strongly negative (ROLE_NEG; the last-but-one
    row), spike on key 0 (ROLE_FIRST: the first tile — with ROLE_TILE the running maximum grows in the last tile, the
    forward's rare re-basing branch), or none."""
    r = np.array([(ROLE_LAST, ROLE_TILE, ROLE_NEG, ROLE_FIRST, ROLE_NORMAL, ROLE_NORMAL)[i % 6] for i in range(Tb)])
    r[Tb - 2] = ROLE_NEG
    r[Tb - 1] = ROLE_LAST
    return r


def probe_inputs(rng, S, H, d, T, nb, T_last=None, ld=None):
    """fp32 maps q (pre-scaled queries), k, v (S, H d, ld) with probe rows in every (slot, head, block) and zeros past the
    last point.  Values, on the eight offset channels OFF of every head: 2 s_c on ordinary keys, 2 s_c b_c on the last valid key,
    2 s_c a_c on the first key of the last tile (s_c random signs, a_c / b_c fixed sign patterns that are -1 on half the
    channels), so that a spike row, an ordinary row (~ +2 s_c) and a row that a padding key took over (~ 0) are O(1) apart
    whichever keys dropout keeps; 0.5 noise on every channel.  (row_inputs gives the output gradient no weight on OFF: the
    offsets would make delta = rowsum(dO * O) large against dS, and its fp32 rounding the kernels' whole error.)"""
    N = n_points(T, nb, T_last)
    ld = N if ld is None else ld
    noise = 0.7 / math.sqrt(math.sqrt(d))
    q = (rng.standard_normal((S, H, d, ld)) * noise).astype(np.float32)
    k = (rng.standard_normal((S, H, d, ld)) * noise).astype(np.float32)
    n_off = len(OFF)
    sgn = np.where(rng.standard_normal((S, H, n_off, 1)) > 0, 1.0, -1.0)
    alt = np.tile([1.0, -1.0], n_off // 2).reshape(n_off, 1)
    alt2 = np.repeat([1.0, -1.0], n_off // 2).reshape(n_off, 1)
    v = (0.5 * rng.standard_normal((S, H, d, ld))).astype(np.float32)
    v[:, :, OFF] += (2.0 * sgn).astype(np.float32)
    for b, Tb in enumerate(block_lengths(T, nb, T_last)):
        c0 = b * T
        kl, kf = probe_keys(Tb)
        roles = query_roles(Tb)
        q[:, :, :4, c0:c0 + Tb] = 0.0
        k[:, :, :4, c0:c0 + Tb] = 0.0
        k[:, :, CH_NEG, c0:c0 + Tb] = NEG_K
        k[:, :, CH_LAST, c0 + kl] = 1.0
        k[:, :, CH_TILE, c0 + kf] = 1.0
        k[:, :, CH_FIRST, c0] = 1.0
        v[:, :, OFF, c0 + kf] = (2.0 * sgn * alt)[..., 0] + 0.5 * rng.standard_normal((S, H, n_off))
        v[:, :, OFF, c0 + kl] = (2.0 * sgn * alt2)[..., 0] + 0.5 * rng.standard_normal((S, H, n_off))
        for role, ch, val in ((ROLE_LAST, CH_LAST, SPIKE), (ROLE_TILE, CH_TILE, SPIKE), (ROLE_NEG, CH_NEG, -SPIKE / NEG_K),
                              (ROLE_FIRST, CH_FIRST, SPIKE)):
            cols = c0 + np.nonzero(roles == role)[0]
            q[:, :, ch, cols] = val
    for t in (q, k, v):
        t[..., N:] = 0.0
    f = lambda t: torch.from_numpy(t.reshape(S, H * d, ld))
    return f(q), f(k), f(v)


def control_gaps(q, k, v, dctx, T, nb, T_last, keep, keep_shifted, p):
    """The negative controls of one row, from the same inputs: per block, the smallest relative ctx difference (relative to
    the block's max |ctx|) of the true reference against
      'last key'  the reference without the last valid key, on the ROLE_LAST rows that keep it;
      'padding'   the reference with one zero padding key let in, on the ROLE_NEG rows that keep some key;
      'shift'     the reference with the keep mask shifted by one key, on the spike rows whose spiked key's keep decision the
                  shift changes (None without dropout or where no such row exists).
    q, k, v, dctx: (E, H, d, N) per evaluation."""
    ref = block_attention_ref(q, k, v, dctx, T, nb, T_last, keep, p)["ctx"]
    ctl = {"last key": block_attention_ref(q, k, v, dctx, T, nb, T_last, keep, p, drop_last_key=True)["ctx"],
           "padding": block_attention_ref(q, k, v, dctx, T, nb, T_last, keep, p, pad_keys=1)["ctx"]}
    if keep is not None:
        ctl["shift"] = block_attention_ref(q, k, v, dctx, T, nb, T_last, keep_shifted, p)["ctx"]
    gaps = {n: [] for n in ("last key", "padding", "shift")}
    for b, Tb in enumerate(block_lengths(T, nb, T_last)):
        c0 = b * T
        roles = query_roles(Tb)
        kl, kf = probe_keys(Tb)
        r = ref[..., c0:c0 + Tb]
        scale = r.abs().amax(dim=(-1, -2), keepdim=True)                # (E, H, 1, 1): the block's max
        # (a row whose keys are all dropped is zero whatever the kernel does with them: it is no probe)
        live = keep[:, :, b, :Tb, :Tb].any(-1).to(r.device) if keep is not None else torch.ones(r.shape[:2] + (Tb,), dtype=torch.bool)
        # (a ROLE_LAST row whose spiked key is dropped probes the mask, not the key: 'shift' below)
        spike_kept = keep[:, :, b, :Tb, kl].to(r.device) if keep is not None else live
        for name, rows, ok in (("last key", roles == ROLE_LAST, spike_kept), ("padding", roles == ROLE_NEG, live)):
            diff = (ctl[name][..., c0:c0 + Tb] - r).abs().amax(-2) / scale[..., 0]      # (E, H, Tb) per query row
            diff = torch.where(ok, diff, torch.full_like(diff, float("inf")))
            gaps[name].append(diff[..., torch.from_numpy(rows)].min().item())
        if keep is not None:
            target = {ROLE_LAST: kl, ROLE_TILE: kf, ROLE_FIRST: 0}
            diff = (ctl["shift"][..., c0:c0 + Tb] - r).abs().amax(-2) / scale[..., 0]
            sel = torch.zeros(diff.shape, dtype=torch.bool)
            for role, key in target.items():
                rows = torch.from_numpy(np.nonzero(roles == role)[0])
                flip = keep[:, :, b, rows, key] != keep_shifted[:, :, b, rows, key]
                sel[..., rows] |= flip
            if sel.any():
                gaps["shift"].append(diff[sel].min().item())
    return {n: (min(g) if g else None) for n, g in gaps.items()}


# ---- the row table --------------------------------------------------------------------------------------------------------
# instance = (math mode, K / V form): 'f32' fp32 K / V maps, 'tp' tile planes (16-bit K / V, required in modes 2 / 3)
INSTANCES = [(0, "f32"), (1, "f32"), (1, "tp"), (2, "tp"), (3, "tp")]
DIMS = (32, 64, 96, 128, 256)
# (block, short last block or None): every block length of the issue, the short last blocks on the multi-tile blocks
BLOCKS = [(4, None), (28, None), (32, None), (64, None), (512, None), (36, 4), (60, 28), (260, 36), (508, 100), (500, None)]
SHORT_LAST = (4, 28, 36, 100)
HIGH_SEED = 0x9e37_79b9_7f4a_7c15          # a seed with its high 32 bits set


def _row(i, mode, kv, d, T, T_last):
    """one row of the sweep: a deterministic mix of the remaining axes over the row index"""
    H = 8 if d == 32 and i % 2 == 0 else (2 if d <= 128 else 1)
    p = (0.0, 0.1, 0.1, 0.5)[i % 4] if mode != 3 else (0.0, 0.1)[i % 2]
    nb = 2 if (T >= 260 or H == 8) else 3
    Tp = ceil_to(T, KT) + (KT if i % 5 == 0 else 0)            # some rows with score_pitch past the round-up of T
    pad = 8 if (T_last is None and i % 3 == 0) else 0            # ld past nb * T: points no block owns
    seed = HIGH_SEED + i if i % 2 else 1000 + 7 * i
    return dict(mode=mode, kv=kv, d=d, H=H, T=T, nb=nb, T_last=T_last, p=p, Tp=Tp, pad=pad, seed=seed,
                S=2, E=3, q_idx=(0, 1, 0), kv_idx=(1, 1, 0))


def rows():
    out = []
    i = 0
    for mode, kv in INSTANCES:
        for d in DIMS:
            for T, T_last in BLOCKS:
                out.append(_row(i, mode, kv, d, T, T_last))
                i += 1
    return out


def row_id(r):
    s = f"m{r['mode']}{r['kv']}-d{r['d']}-H{r['H']}-T{r['T']}x{r['nb']}"
    if r["T_last"]:
        s += f"-last{r['T_last']}"
    return s + f"-p{r['p']}-Tp{r['Tp']}"


# csn_attn_bwd_grouping (csn_capi.hip) restated as data: bit 0 grouped dQ, 1 grouped dK / dV products, 2 dQ recompute,
# 3 flash dK / dV, 4 tile-major scores
def grouping(mode, d, T):
    if mode == 0:
        return 0
    bk4 = ceil_to(T, 4)
    tiles_ok = mode != 3 and T <= 512 and T % 4 == 0 and d in DIMS
    recompute = tiles_ok and (mode != 1 or d // 32 <= 4)              # csn_attn_recompute_fits: one plane, or two up to d = 128
    flash = recompute and d // 32 <= 4                                # csn_attn_dkv_flash_fits
    big = d >= 192 and bk4 >= 224                                     # csn_gemm_bf16x3_big_tiles (big tiles on by default)
    tm = mode == 1 and tiles_ok and big                               # csn_gemm_tile_major_planes (wide GEMM on by default)
    return 1 | (2 if big else 0) | (4 if recompute else 0) | (8 if flash else 0) | (16 if tm else 0)


def forms(r):
    """every call form the library offers for the row (what the GPU sweep runs)"""
    mode, g = r["mode"], grouping(r["mode"], r["d"], r["T"])
    f = {"fwd", "fwd_noscores"}
    if mode == 3:
        return f
    tp = r["kv"] == "tp"
    if mode == 0 or not tp:
        f |= {"dq", "dkv"}
    else:
        f |= {"dq_tiles", "dq_grouped", "dkv_tiles"}
        if g & 2:
            f.add("dkv_grouped")
        if g & 4:
            f |= {"dq_recompute", "dq_recompute_grouped"}
        if g & 8:
            f |= {"flash", "flash_grouped", "flash_colours"}
        if g & 16:
            f.add("tile_major")
    return f


# ---- inputs and bounds of one row -------------------------------------------------------------------------------------------
FMT = {0: None, 1: None, 2: "bf16", 3: "f16"}
# per-block bounds of the modes: (forward outputs ctx / lse / S / P, gradients dS / delta / dQ / dK / dV).  Mode 0: fp32 rounding
# (tests/test_gpu_dropout.py); mode 1: the 1e-4 contract's kernels; modes 2 / 3 against operands rounded to the mode's 16 bits
# (the P / dS operands are rounded once more inside: 2^-9 relative)
BOUNDS = {0: (5e-6, 2e-5), 1: (2e-4, 2e-4), 2: (1e-2, 3e-2), 3: (1e-2, 3e-2)}


def row_inputs(r):
    """fp32 slot maps q, k, v (S, H d, ld) and dctx (E, H d, ld) of a row (zeros past the last point); in the one-plane modes
    every operand already holds a value of the mode's 16 bits (the kernels' own rounding of them is then exact)."""
    rng = np.random.default_rng(r["seed"] & 0xffffffff)
    T, nb, Tl = r["T"], r["nb"], r["T_last"]
    N = n_points(T, nb, Tl)
    ld = N + r["pad"]
    q, k, v = probe_inputs(rng, r["S"], r["H"], r["d"], T, nb, Tl, ld)
    dctx = torch.from_numpy(rng.standard_normal((r["E"], r["H"] * r["d"], ld)).astype(np.float32))
    dctx[..., N:] = 0.0
    dctx.view(r["E"], r["H"], r["d"], ld)[:, :, OFF] = 0.0
    # no output gradient on the spike rows: there P is one-hot to ~1e-3 and dS = P (dP - delta) is a difference of two nearly
    # equal numbers whose fp32 rounding (delta = rowsum(dO * O), |O| ~ |v|) would be all the kernel's error; the backward's
    # probes of those rows are the P it writes
    for b, Tb in enumerate(block_lengths(T, nb, Tl)):
        spike = np.nonzero(np.isin(query_roles(Tb), (ROLE_LAST, ROLE_TILE, ROLE_FIRST)))[0]
        dctx[..., b * T + spike] = 0.0
    fmt = FMT[r["mode"]]
    q, k, v, dctx = (round16(t, fmt) for t in (q, k, v, dctx))
    return q, k, v, dctx


def per_eval(x, idx, H):
    """slot maps (S, H d, ld) -> per-evaluation (E, H, d, ld) float64"""
    x = x[list(idx)].double()
    return x.view(x.shape[0], H, -1, x.shape[-1])


def row_masks(r):
    """(keep, keep shifted by one key) of a row, or (None, None) without dropout"""
    if r["p"] <= 0:
        return None, None
    ext = block_keep(r["E"], r["H"], r["T"], r["nb"], r["Tp"], r["seed"], r["p"], extra_keys=1)
    return ext[..., :r["T"]].contiguous(), ext[..., 1:].contiguous()
