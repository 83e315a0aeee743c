"""Host infrastructure of the cross-length / ragged attention sweep (tests/test_gpu_cross_attn_edges.py,
tests/test_cpu_cross_attn_edges.py) on top of tests/attn_edge_ref.py: the entry points of sections (3b) and (3c) of
include/csn_hip.h — one unchunked block per evaluation, n_queries != n_keys, key counts that are no multiples of 4.

- cross_attention_ref: attention_core per evaluation with its own (nq[e], nk[e]) — float64, or float32 for the err32 yardstick.
- launch_keep: the keep mask of a launch, drawn with the LAUNCH's query count and score pitch.
- cross_inputs: rectangular probe inputs (the roles of attn_edge_ref.query_roles) whose padding columns hold finite SENTINELS
  instead of zeros: the header only asks the padding points of the input maps to be finite, so reading one as data must be
  an O(1) error, not a silent zero.
- The row tables of (3b) and (3c) as data, and the written regions of every output restated from the header as boolean masks.
"""
import math

import numpy as np
import torch

from tests import attn_edge_ref as ar
from tests import dropout_ref as dr

ceil_to = ar.ceil_to
KT = ar.KT

# ---- sentinels ------------------------------------------------------------------------------------------------------------
# Two sets (the second one for the "padding is not read as data" rerun).  A padding KEY scores +SPIKE for the probe rows whose
# real keys are all strongly negative (CH_NEG: query -SPIKE / NEG_K times key -NEG_K) and ties with the spiked key of every
# spike row (1 on the three spike channels); a padding VALUE is far from every real value (|v| <~ 4).
SENTINELS = [dict(k_neg=-ar.NEG_K, k_spike=1.0, k_other=0.0, v=7.0, q=3.0, ctx=5.0, dctx=-4.0, lse=2.5),
             dict(k_neg=-2 * ar.NEG_K, k_spike=1.5, k_other=0.125, v=-9.0, q=-1.5, ctx=-6.0, dctx=2.0, lse=-1.25)]


def key_sentinel(H, d, which=0):
    """(k, v) columns (H, d) of one padding key"""
    s = SENTINELS[which]
    k = torch.full((H, d), s["k_other"], dtype=torch.float32)
    k[:, ar.CH_NEG] = s["k_neg"]
    for ch in (ar.CH_LAST, ar.CH_TILE, ar.CH_FIRST):
        k[:, ch] = s["k_spike"]
    return k, torch.full((H, d), s["v"], dtype=torch.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def cross_inputs(r, which=0):
    """fp32 maps of a row: q, dctx (E, H d, ld_q), k, v (E, H d, ld_kv).  Evaluation e holds nq[e] queries with the roles of
    attn_edge_ref.query_roles(nq[e]) and nk[e] keys whose probe keys are nk - 1, the first key of the last 32-key tile and key
    0 (they coincide for short rows, down to nk = 1); values and output gradient as attn_edge_ref.probe_inputs / row_inputs:
    offsets on the channels OFF, no output gradient on OFF or on the spike rows.  Every column past an evaluation's own count
    holds the sentinel of set `which`; the real columns do not depend on `which`.  r["redraw"] selects another draw of the
    random part (REDRAW below)."""
    E, H, d, ld_q, ld_kv = r["E"], r["H"], r["d"], r["ld_q"], r["ld_kv"]
    rng = np.random.default_rng([r["seed"] & 0xffffffff, r.get("redraw", 0)])
    sen = SENTINELS[which]
    noise = 0.7 / math.sqrt(math.sqrt(d))
    n_off = len(ar.OFF)
    alt = np.tile([1.0, -1.0], n_off // 2)
    alt2 = np.repeat([1.0, -1.0], n_off // 2)
    q = np.full((E, H, d, ld_q), sen["q"], dtype=np.float32)
    dctx = np.full((E, H, d, ld_q), sen["dctx"], dtype=np.float32)
    k = np.empty((E, H, d, ld_kv), dtype=np.float32)
    v = np.empty((E, H, d, ld_kv), dtype=np.float32)
    ks, vs = key_sentinel(H, d, which)
    k[:] = ks.numpy()[None, :, :, None]
    v[:] = vs.numpy()[None, :, :, None]
    for e in range(E):
        nq, nk = r["nq"][e], r["nk"][e]
        roles = ar.query_roles(nq)
        kl, kf = ar.probe_keys(nk)
        qe = (rng.standard_normal((H, d, nq)) * noise).astype(np.float32)
        ke = (rng.standard_normal((H, d, nk)) * noise).astype(np.float32)
        ve = (0.5 * rng.standard_normal((H, d, nk))).astype(np.float32)
        sgn = np.where(rng.standard_normal((H, n_off, 1)) > 0, 1.0, -1.0)
        ve[:, ar.OFF] += (2.0 * sgn).astype(np.float32)
        qe[:, :4] = 0.0
        ke[:, :4] = 0.0
        ke[:, ar.CH_NEG] = ar.NEG_K
        ke[:, ar.CH_LAST, kl] = 1.0
        ke[:, ar.CH_TILE, kf] = 1.0
        ke[:, ar.CH_FIRST, 0] = 1.0
        ve[:, ar.OFF, kf] = 2.0 * sgn[..., 0] * alt + 0.5 * rng.standard_normal((H, n_off))
        ve[:, ar.OFF, kl] = 2.0 * sgn[..., 0] * alt2 + 0.5 * rng.standard_normal((H, n_off))
        for role, ch, val in ((ar.ROLE_LAST, ar.CH_LAST, ar.SPIKE), (ar.ROLE_TILE, ar.CH_TILE, ar.SPIKE),
                              (ar.ROLE_NEG, ar.CH_NEG, -ar.SPIKE / ar.NEG_K), (ar.ROLE_FIRST, ar.CH_FIRST, ar.SPIKE)):
            qe[:, ch, np.nonzero(roles == role)[0]] = val
        de = rng.standard_normal((H, d, nq)).astype(np.float32)
        de[:, ar.OFF] = 0.0
        de[:, :, np.nonzero(np.isin(roles, (ar.ROLE_LAST, ar.ROLE_TILE, ar.ROLE_FIRST)))[0]] = 0.0
        q[e, :, :, :nq], dctx[e, :, :, :nq] = qe, de
        k[e, :, :, :nk], v[e, :, :, :nk] = ke, ve
    f = lambda t, ld: torch.from_numpy(t.reshape(E, H * d, ld))
    return f(q, ld_q), f(k, ld_kv), f(v, ld_kv), f(dctx, ld_q)


# ---- masks and reference ----------------------------------------------------------------------------------------------------
def launch_keep(E, H, n_queries, n_keys, Tp, seed, p, mask_pitch=None, shift=0):
    """keep[e][h][query][key] (bool, torch) of a launch whose scores are [E][H][n_queries][Tp]: dropout_ref.attention_mask with
    one block, Tq = the LAUNCH's query count (n_queries of (3b), max_queries of (3c)) and the launch's score pitch — the pair
    index is key / 2 * max(Tp, Tq) + query.  mask_pitch: draw with another pitch (the wrong-pitch controls); shift = 1: the
    mask of the keys 1 .. n_keys (the shifted-mask control)."""
    if p <= 0:
        return None
    m = dr.attention_mask(E, H, 1, n_keys + shift, Tp, seed, p, Tq=n_queries, pitch=mask_pitch)[:, :, 0]     # [e][h][key][query]
    return torch.from_numpy(np.ascontiguousarray(m[:, :, shift:].transpose(0, 1, 3, 2)))


def row_keep(r, **kw):
    return launch_keep(r["E"], r["H"], max(r["nq"]), max(r["nk"]), r["Tp"], r["seed"], r["p"], **kw)


def cross_attention_ref(q, k, v, dctx, nq, nk, keep=None, p=0.0, dtype=torch.float64, grads=True, drop_last_key=False,
                        pad_key=None):
    """The reference of a launch: q, dctx (E, H, d, >= nq[e]), k, v (E, H, d, >= nk[e]); keep [E][H][>= nq][>= nk] or None.
    Returns one dict per evaluation (attention_core's: ctx, lse, S, P, dS, delta, dq, dk, dv) cut to the evaluation's own
    (nq[e], nk[e]).  Controls: drop_last_key removes key nk[e] - 1; pad_key = (k, v) columns (H, d) lets one more key in."""
    scale = 1.0 / (1.0 - p) if keep is not None else 1.0
    out = []
    for e in range(q.shape[0]):
        n, m = nq[e], nk[e] - (1 if drop_last_key else 0)
        ek = ev = None
        if pad_key is not None:
            ek, ev = (t.to(q.device).unsqueeze(-1) for t in pad_key)
        out.append(ar.attention_core(q[e, :, :, :n], k[e, :, :, :m], v[e, :, :, :m], dctx[e, :, :, :n],
                                     keep[e, :, :n, :m] if keep is not None else None, scale, ek, ev, grads, dtype))
    return out


def eval_err(got, ref, scale=None):
    """max over heads of max|got - ref| / max|ref| of one evaluation (first dimension: heads) — an error confined to one
    evaluation or head is never diluted by its neighbours.  scale (per head, or a number): the denominator where the
    reference is exactly zero.  NaN in got (never written, or a NaN read) is an infinite error."""
    got, ref = got.double(), ref.double().to(got.device)
    H = ref.shape[0]
    diff = (got - ref).abs().reshape(H, -1)
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    den = ref.abs().reshape(H, -1).amax(-1) if scale is None else torch.as_tensor(scale, dtype=torch.float64, device=got.device)
    return (diff.amax(-1) / den.clamp_min(1e-30)).max().item()


def zero_scales(q, k, v, dctx, n, m):
    """natural scales (per head) of dS, dQ, dK of a one-key evaluation, where the reference is exactly zero: max|dO^T V| for
    dS, times max|k| for dQ, times max|q| for dK (float64, from the inputs)."""
    qe, ke, ve, de = (t.double() for t in (q[:, :, :n], k[:, :, :m], v[:, :, :m], dctx[:, :, :n]))
    ds = (de.transpose(-1, -2) @ ve).abs().amax((-1, -2))
    return {"dS": ds, "dq": ds * ke.abs().amax((-1, -2)), "dk": ds * qe.abs().amax((-1, -2))}


# ---- conditioning of a draw ---------------------------------------------------------------------------------------------------
# Errors are taken relative to max |reference| of one (evaluation, head).  With one key pair or one 4-query group a whole
# gradient can come out small by chance — dS = P0 P1 (dP0 - dP1) of the single row that carries an output gradient, or
# dK[CH_NEG] = -48 * (sum of dS over the all-negative rows) cancelling to 1 / 800 of its terms — and then max |reference| no
# longer measures the size of what the kernel adds up: fp32 rounding of the terms alone exceeds any relative bound.  Such a
# draw tests the dice, not the kernel.  condition() measures it from the float64 reference ALONE: for every gradient, the
# largest sum of |terms| of its last contraction over max |result|, divided by sqrt(number of terms) (what a sum of random
# signs loses anyway).  Typical draws give 0.3 .. 2; a draw above COND_LIMIT is replaced by the next one (REDRAW, checked by
# tests/test_cpu_cross_attn_edges.py and asserted again by the GPU sweep for every row).
COND_LIMIT = 8.0


def condition(ref, q, k, v, dctx, keep_scale=None):
    """{gradient: worst condition over the heads} of one evaluation: ref = attention_core's dict, q, dctx (H, d, nq), k, v
    (H, d, nk) float64, keep_scale (H, nq, nk) = mask / (1 - p) or None.  Gradients that are exactly zero are left out."""
    P_soft = torch.exp(ref["S"] - ref["lse"].unsqueeze(-1))
    dP = dctx.transpose(-1, -2) @ v
    if keep_scale is not None:
        dP = dP * keep_scale
    dS, P = ref["dS"].abs(), ref["P"].abs()
    nq, nk = dS.shape[-2:]
    terms = {"dS": ((P_soft * (dP.abs() + ref["delta"].abs().unsqueeze(-1))).amax((-1, -2)), 2),
             "dq": ((k.abs() @ dS.transpose(-1, -2)).amax((-1, -2)), nk),
             "dk": ((q.abs() @ dS).amax((-1, -2)), nq),
             "dv": ((dctx.abs() @ P).amax((-1, -2)), nq)}
    out = {}
    for n, (t, count) in terms.items():
        top = ref[n].abs().amax((-1, -2))
        if float(top.max()) == 0.0:
            continue
        out[n] = float((t / top.clamp_min(1e-300)).max()) / math.sqrt(count)
    return out


def row_condition(r, ref, q, k, v, dctx, keep):
    """worst condition() over the evaluations of a row (inputs (E, H, d, ld) float64 on the reference's device)"""
    worst = {}
    for e in range(r["E"]):
        n, m = r["nq"][e], r["nk"][e]
        ks = keep[e, :, :n, :m].to(q.device).double() / (1.0 - r["p"]) if keep is not None else None
        for name, c in condition(ref[e], q[e, :, :, :n], k[e, :, :, :m], v[e, :, :, :m], dctx[e, :, :, :n], ks).items():
            worst[name] = max(worst.get(name, 0.0), c)
    return worst


# row index -> draw, for the rows whose first draw(s) are ill-conditioned
REDRAW = {15: 2, 19: 1}


# ---- the row tables -----------------------------------------------------------------------------------------------------------
DIMS = ar.DIMS
KEY_COUNTS = (1, 2, 3, 5, 31, 32, 33, 37, 63, 64, 65, 100, 511, 512, 513, 1301)
QUERY_COUNTS = (4, 8, 124, 128, 132, 260)
MANY_QUERIES = 1000                      # paired with key counts whose score pitch is below it: mask pitch = query count
PITCHES = ("r4", "r32", "r32+32")        # round-up-4(nk): fp32 P / dS rows in mode 1; round-up-32: tile planes; one tile more
HIGH_SEED = ar.HIGH_SEED


KEY_CLASSES = ("below one 4-run", "around one tile", "a few tiles", "around the block path's limit", "many tiles")


def key_class(nk):
    """the class of a key count"""
    if nk <= 5:
        return KEY_CLASSES[0]
    if nk <= 37:
        return KEY_CLASSES[1]
    if nk <= 100:
        return KEY_CLASSES[2]
    return KEY_CLASSES[3] if nk <= 513 else KEY_CLASSES[4]


def pitch_of(cls, nk):
    return {"r4": ceil_to(nk, 4), "r32": ceil_to(nk, KT), "r32+32": ceil_to(nk, KT) + KT}[cls]


def planes_flow(mode, Tp, nk_max):
    """csn_capi.hip: in math mode 1 the backward leaves P / dS as bf16 tile planes from score_pitch = round-up-32(n_keys) on,
    as fp32 rows below (mode 0: always fp32 rows)"""
    return mode != 0 and Tp >= ceil_to(nk_max, KT)


def _finish(r, i, mix):
    """the secondary axes shared by (3b) and (3c): leading dimensions, strides, dropout, seed — a deterministic mix over `mix`
    (chosen so that every (mode, head width) walks through all of them); i: the row's index in its table"""
    H, d = r["H"], r["d"]
    nq_max, nk4 = max(r["nq"]), ceil_to(max(r["nk"]), 4)
    r["ld_q"] = nq_max + (8 if mix % 3 == 1 else 0)
    r["ld_kv"] = nk4 + (12 if mix % 3 != 0 else 0)
    r["q_stride"] = H * d * r["ld_q"] + (16 if mix % 4 >= 2 else 0)
    r["kv_stride"] = H * d * r["ld_kv"] + (32 if mix % 4 in (1, 2) else 0)
    r["p"] = (0.0, 0.1, 0.1, 0.5)[mix % 4]
    r["seed"] = HIGH_SEED + i if mix % 2 else 1000 + 7 * i
    r["i"] = i
    r["redraw"] = REDRAW.get(i, 0)
    return r


def _heads(d, i):
    return 8 if (d == 32 and i % 2 == 0) else (2 if d <= 128 else 1)


def cross_rows():
    """(3b): math modes 0 and 1 x head width x key count, the other axes mixed over the row index; the largest rows last"""
    out = []
    i = 0
    for ik, nk in enumerate(KEY_COUNTS):
        for idd, d in enumerate(DIMS):
            for mode in (0, 1):
                pc = PITCHES[(ik + idd) % 3]
                nq = QUERY_COUNTS[(ik + 2 * idd + mode) % len(QUERY_COUNTS)]
                if (nk == 37 and d in (32, 128)) or (nk == 5 and d == 64) or (nk == 1301 and d in (32, 256)):
                    nq = MANY_QUERIES
                E = 2 + (ik + idd) % 2
                r = dict(kind="cross", mode=mode, d=d, H=_heads(d, ik), E=E, nq=[nq] * E, nk=[nk] * E, pitch=pc,
                         Tp=pitch_of(pc, nk))
                out.append(_finish(r, i, 7 * ik + 3 * idd + mode))
                i += 1
    return out


# (3c) batches: all query counts and all key counts of a batch differ; one evaluation with a single key, one with a single
# 4-query group, one with several query tiles; the longest (most keys, and most queries) not first
BATCHES = [dict(nq=(128, 4, 260, 8, 124), nk=(33, 100, 1, 65, 5)),                  # max_queries 260 > either pitch class
           dict(nq=(8, 388, 4, 132, 124, 12), nk=(37, 3, 513, 1, 64, 31)),
           dict(nq=(12, 1000, 4, 128, 8), nk=(1, 37, 2, 57, 32)),                    # max_queries 1000 on a pitch of 60 / 64
           dict(nq=(132, 8, 516, 4, 128), nk=(511, 1301, 1, 65, 512))]
VARLEN_PITCHES = ("r4", "r32")


def varlen_rows():
    out = []
    i = 0
    for b, batch in enumerate(BATCHES):                                     # (the batch with 1301 keys last)
        for idd, d in enumerate(DIMS):
            for mode in (0, 1):
                for ipc, pc in enumerate(VARLEN_PITCHES):
                    if (idd + 2 * ipc + mode) % len(BATCHES) != b:
                        continue
                    E = len(batch["nq"])
                    r = dict(kind="varlen", mode=mode, d=d, H=_heads(d, i), E=E, nq=list(batch["nq"]), nk=list(batch["nk"]),
                             pitch=pc, Tp=pitch_of(pc, max(batch["nk"])))
                    out.append(_finish(r, 300 + i, i))
                    i += 1
    return out


def row_id(r):
    if r["kind"] == "cross":
        shape = f"q{r['nq'][0]}-k{r['nk'][0]}-E{r['E']}"
    else:
        shape = f"batch{BATCHES.index(dict(nq=tuple(r['nq']), nk=tuple(r['nk'])))}"
    return f"{r['kind']}-m{r['mode']}-d{r['d']}-H{r['H']}-{shape}-Tp{r['Tp']}-p{r['p']}-i{r['i']}"


def other_mode_rows():
    """the rows that are also run in math modes 2 and 3 (which run as mode 1, bit for bit): (3b) and (3c), both data flows"""
    c = [r for r in cross_rows() if r["mode"] == 1]
    picks = [c[j] for j in (3, 17, 22, 36, 41, 55, 68)]
    return picks + [r for r in varlen_rows() if r["mode"] == 1][:3]


def resentinel_rows():
    """the rows run a second time with the other sentinel set: rows with padding keys, every 12th of them"""
    padded = [r for r in cross_rows() if r["ld_kv"] > r["nk"][0]]
    return padded[5::12] + [r for r in varlen_rows() if r["i"] % 7 == 0]


# ---- the written regions, restated from include/csn_hip.h (3b) / (3c) ------------------------------------------------------------
def map_written(r, keys, device="cpu"):
    """q-side maps (ctx, dq: keys = False) [E][q_stride]: the columns < nq[e] of the n_heads * d_head rows of pitch ld_q;
    key-side maps (dk, dv: keys = True) [E][kv_stride]: the columns < round-up-4(nk[e]) — the products store 16-byte runs and
    the columns nk .. round-up-4(nk) are exact zeros.  Everything else — the rest of a row up to ld, the elements between
    n_heads * d_head * ld and the stride — is left alone."""
    D = r["H"] * r["d"]
    ld, stride = (r["ld_kv"], r["kv_stride"]) if keys else (r["ld_q"], r["q_stride"])
    m = torch.zeros((r["E"], stride), dtype=torch.bool, device=device)
    for e in range(r["E"]):
        n = ceil_to(r["nk"][e], 4) if keys else r["nq"][e]
        m[e, :D * ld].view(D, ld)[:, :n] = True
    return m


def stat_written(r, device="cpu"):
    """lse, delta [E][H][n_queries]: the entries < nq[e]"""
    m = torch.zeros((r["E"], r["H"], max(r["nq"])), dtype=torch.bool, device=device)
    for e in range(r["E"]):
        m[e, :, :r["nq"][e]] = True
    return m


def score_written(r, planes, device="cpu"):
    """scores / dscores [E][H][n_queries][Tp]: the rows < nq[e]; fp32 rows: the columns < round-up-4(nk[e]) (16-byte runs: the
    columns nk .. round-up-4(nk) MAY be written — -inf by the forward, 0 by the backward); tile planes (mode 1, Tp >=
    round-up-32): every 32-key tile that holds a key, its padding keys written as zeros."""
    m = torch.zeros((r["E"], r["H"], max(r["nq"]), r["Tp"]), dtype=torch.bool, device=device)
    for e in range(r["E"]):
        m[e, :, :r["nq"][e], :ceil_to(r["nk"][e], KT if planes else 4)] = True
    return m


def score_must(r, device="cpu"):
    """the part of score_written (fp32 rows) that MUST be written: the columns < nk[e]"""
    m = torch.zeros((r["E"], r["H"], max(r["nq"]), r["Tp"]), dtype=torch.bool, device=device)
    for e in range(r["E"]):
        m[e, :, :r["nq"][e], :r["nk"][e]] = True
    return m
