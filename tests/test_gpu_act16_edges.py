"""The 16-bit activation-map instances (csn_set_thread_act16; include/csn_hip.h "16-BIT ACTIVATION MAPS") at the edges of their
tiles, through the raw C ABI, BIT FOR BIT against the fp32-map call fed the same 16-bit values: a map that is only a matrix
operand was rounded to those 16 bits at staging anyway, so lse, kept scores, delta, the [P | dS] planes, dQ, dK, dV, dz_res and
dW_fc must be the same bits and every 16-bit output the fp32 output rounded once.  The fp32-map side is held to float64 (the
attention rows within attn_edge_ref.BOUNDS[2], the out-projection + LayerNorm within the bounds DERIVED in tests/act16_ref.py), so
equality carries those bounds over.  16-bit outputs lie in canary buffers sized for the fp32 map (a write of fp32 width shows up),
16-bit inputs hold NaN past their last point and between slots.

Measured on an MI355X (every case prints its figures):
- 5337 bit-identical comparisons of whole buffers, guards included, hold: 4972 over the 150 attention cases (forward with and
  without kept scores; dQ kept-scores / recomputing, per evaluation / grouped, with and without the planes; dK / dV products and
  flash, per evaluation / grouped; each on fmt f and f + 4), 320 + 40 + 5 over the out-projection + LayerNorm cases.
- fp32-map side of the attention rows against float64, worst per-block error (bounds 1e-2 forward, 3e-2 gradients): bf16 forward
  ctx 1.6e-3, lse 4.8e-7, S 5.4e-7, P 3.5e-3, dS 6.0e-3, dQ 6.8e-3, dK 1.1e-2, dV 3.6e-3; fp16 forward / bf16 backward on fp16
  K / V planes ctx 2.6e-4, lse 4.9e-7, S 5.6e-7, P 3.5e-3, dS 3.8e-3, dQ 4.7e-3, dK 1.2e-2, dV 3.6e-3.
  (delta is not held to float64 by itself: a block of 4 points has ONE row with a gradient, so an error relative to the block's
  largest delta has no scale; it is held by bits between the twins and through dQ, dK and dS.)
- out-projection + LayerNorm, worst error / derived bound over the ten shapes and both modes: xhat 0.022, rstd 0.020, xhat_sum
  0.006 (with and without the workspace), xhat_sum on fp16 maps 0.146, dz 0.200, dz_res 0.181, dCtx 0.041, dW_fc 0.098.
- csn_project_f32 writing a 16-bit map: error / bound 0.958 (fp16), 0.988 (bf16) — the bound is the rounding itself.
Before the fix of csrc/outproj_ln.hip that came with this file the small out-projection kernel's rstd differed
from its fp32-map twin in the last bit at about 1 point in 100 and xhat16 from fp16(xhat32) at about 1 element in 1000, both at
0.02 of the derived bound; every other comparison held as it stood."""
import pytest
import torch

from tests import act16_ref as a16
from tests import attn_edge_ref as ar
from tests import test_gpu_attn_edges as ae

pytestmark = pytest.mark.gpu

ROWS2 = [r for r in ar.rows() if r["mode"] == 2 and r["kv"] == "tp"]
Canary = ar.Canary
E_ARG = -1


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_thread_act16(0)
    L.lib().csn_set_thread_score_layout(0)
    L.lib().csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Flags:
    """math mode + exchange format of one call"""

    def __init__(self, L, mode, fmt):
        from csn_amd import functional as CF
        self.L, self.mode, self.ctx = L, mode, CF.act16(fmt)

    def __enter__(self):
        self.L.check(self.L.lib().csn_set_math_mode(self.mode))
        self.ctx.__enter__()

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


def _put32(x, n_valid, stride, ld=None):
    """fp32 maps (n, R, >= n_valid) -> (n, stride) of row pitch ld (None: the maps') with NaN past the last point and between slots"""
    n, R = x.shape[:2]
    ld = x.shape[2] if ld is None else ld
    buf = torch.full((n, stride), float("nan"), device="cuda")
    buf[:, :R * ld].view(n, R, ld)[..., :n_valid] = x[..., :n_valid].cuda()
    return buf


def _put16(x, n_valid, stride, fmt, ld=None):
    """the same maps as ONE 16-bit plane: (n, stride) int16, the same element strides, 16-bit NaN everywhere else"""
    n, R = x.shape[:2]
    ld = x.shape[2] if ld is None else ld
    nan = a16.nan16(fmt)
    buf = torch.full((n, stride), nan - 65536 if nan > 32767 else nan, dtype=torch.int16, device="cuda")
    buf[:, :R * ld].view(n, R, ld)[..., :n_valid] = a16.bits16(x[..., :n_valid].cuda(), fmt)
    return buf


def _vals16(c, n, stride, R, ld, fmt):
    """the 16-bit map a call wrote into canary c -> int16 bits (n, R, ld)"""
    return c.body.view(torch.int16)[:n * stride].view(n, stride)[:, :R * ld].view(n, R, ld)


class _Count:
    bits = 0


def _same(a, b, what):
    assert torch.equal(a.buf, b.buf), f"{what}: the 16-bit call differs from its fp32-map twin"
    _Count.bits += 1


def _rounded(c16, c32, n, slots, stride, R, ld, N, fmt, what):
    """c16 holds, as one 16-bit plane, the map of c32 rounded once; nothing else of its buffer is touched"""
    bad = a16.touched16(c16.body, a16.map_written16(n, slots, stride, R, ld, N, "cuda"))
    assert bad == 0, f"{what}: {bad} 16-bit elements outside the map were written"
    g = torch.cat((c16.buf[:ar.GUARD], c16.buf[ar.GUARD + c16.n:]))
    assert bool((g == ar.CANARY32).all()), f"{what}: a guard was written"
    sl = list(slots)
    got = _vals16(c16, n, stride, R, ld, fmt)[sl][..., :N]
    want = a16.bits16(c32.f32().view(n, stride)[:, :R * ld].view(n, R, ld)[sl][..., :N], fmt)
    assert torch.equal(got, want), f"{what}: not the fp32 map rounded once to {fmt}"
    _Count.bits += 1


def _attention_row(L, r, fwd_mode, fmts, inputs, check_ref):
    """One geometry: the forward in fwd_mode (2: bf16, 3: fp16 K / V planes), every backward form in math mode 2, on fp32 maps and —
    for each fmt of fmts — on 16-bit maps.  check_ref: the fp32-map side against float64 within BOUNDS[2].  With fmts the fp32
    side's backward is fed Ctx16 widened (the same values as the 16-bit side), without it its own fp32 Ctx."""
    lib = L.lib()
    S, E, H, d, T, nb, Tl, Tp, p, seed = (r[n] for n in ("S", "E", "H", "d", "T", "nb", "T_last", "Tp", "p", "seed"))
    L.check(lib.csn_set_math_mode(2))
    grouping = lib.csn_attn_bwd_grouping(d, T)
    assert grouping == ar.grouping(2, d, T)
    forms = ar.forms(r)
    D, N = H * d, ar.n_points(T, nb, Tl)
    ld, nbT = N + r["pad"], nb * T
    fb, bb = ar.BOUNDS[2]
    q, k, v, dctx = inputs
    q_idx, kv_idx = r["q_idx"], r["kv_idx"]
    qi = torch.tensor(q_idx, dtype=torch.int32, device="cuda")
    ki = torch.tensor(kv_idx, dtype=torch.int32, device="cuda")
    f16 = fwd_mode == 3
    tfmt = "f16" if f16 else "bf16"                      # the forward's 16-bit type
    ffmt = 2 if f16 else 1                               # ... as the flag names it
    kv_split = 2 if f16 else 1
    mstride = cstride = dq_stride = D * ld + 16
    q32, d32 = _put32(q, N, mstride), _put32(dctx, N, mstride)
    q16, d16 = _put16(q, N, mstride, tfmt), _put16(dctx, N, mstride, "bf16")
    ldp = nb * ar.BLOCK_PITCH
    planes = ar.pack_tile_planes(torch.cat((k, v), 1), T, nb, 1, tfmt, Tl)
    kvs = 2 * D * ldp + 64
    kvbuf = torch.full((S, kvs), a16.nan16(tfmt), dtype=torch.int16, device="cuda")
    kvbuf[:, :2 * D * ldp] = planes.reshape(S, -1).cuda()
    k_ptr, v_ptr = kvbuf.data_ptr(), kvbuf.data_ptr() + 2 * D * ldp
    qp = lambda fmt: (q16 if fmt else q32).data_ptr()
    dp = lambda fmt: (d16 if fmt else d32).data_ptr()
    maps = lambda c, n: c.f32().view(n, -1)[:, :D * ld].view(n, H, d, ld)
    ctx_w = a16.map_written(E, range(E), cstride, D, ld, N, "cuda")
    stat_w = ae._stat_written(E, H, nbT, N)
    errs = {}

    ref = None
    if check_ref:
        keep, _ = ar.row_masks(r)
        ref = ar.block_attention_ref(*(ar.per_eval(t, ix, H).cuda() for t, ix in ((q, q_idx), (k, kv_idx), (v, kv_idx))),
                                     dctx.double().view(E, H, d, ld).cuda(), T, nb, Tl, keep, p)

    def err(name, got, want, bound):
        if ref is None:
            return
        e = ar.per_block_err(got, want, T, nb, Tl)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e < bound, f"{name}: per-block error {e:.3e} >= {bound:.1e} (fp32-map side)"

    def slot_ref(name, idx, n_slots):
        out = torch.zeros((n_slots, H, d, ld), dtype=torch.float64, device="cuda")
        return out.index_add_(0, torch.tensor(idx, device="cuda"), ref[name])

    # ---- forward: lse and kept scores the same bits, Ctx16 = the fp32 Ctx rounded once; with and without kept scores
    def forward(fmt, keep_scores):
        ctx, lse = Canary(E * cstride), Canary(E * H * nbT)
        sc = Canary(E * H * nbT * Tp) if keep_scores else None
        with _Flags(L, fwd_mode, fmt):
            L.check(lib.csn_block_attn_fwd_f32(qp(fmt), k_ptr, v_ptr, mstride, kvs, qi.data_ptr(), ki.data_ptr(), ld, ctx.ptr,
                                               cstride, sc.ptr if sc else None, lse.ptr, E, H, d, T, nb, Tp, 8.0, p, seed, 1, ldp,
                                               _stream()), "forward")
        return ctx, lse, sc

    ctx32, lse, sc = forward(0, True)
    ctx32.check(ctx_w, "ctx")
    lse.check(stat_w, "lse")
    sc.check(ae._score_written(r, False), "scores")
    err("ctx", maps(ctx32, E), ref and ref["ctx"], fb)
    err("lse", lse.f32().view(E, H, nbT), ref and ref["lse"], fb)
    err("S", ae._decode_scores(sc, r)[..., :T], ref and ref["S"], fb)
    c32n, lse_n, _ = forward(0, False)
    assert torch.equal(c32n.buf, ctx32.buf) and torch.equal(lse_n.buf, lse.buf), "forward differs without kept scores"
    ctx16 = None
    if fmts:
        for keep_scores in (True, False):
            ctx16, lse16, sc16 = forward(ffmt, keep_scores)
            _same(lse16, lse, "lse")
            if keep_scores:
                _same(sc16, sc, "kept scores")
            _rounded(ctx16, ctx32, E, range(E), cstride, D, ld, N, tfmt, "Ctx16")
        ctx_feed = torch.full((E, cstride), float("nan"), device="cuda")       # Ctx16 widened: what the fp32 side is fed
        ctx_feed[:, :D * ld].view(E, D, ld)[..., :N] = a16.widen16(_vals16(ctx16, E, cstride, D, ld, tfmt)[..., :N], tfmt)
        cp = lambda fmt: ctx16.ptr if fmt else ctx_feed.data_ptr()
    else:
        cp = lambda fmt: ctx32.ptr
    sc_before = sc.buf.clone()

    # ---- backward, math mode 2 (K / V planes of an fp16 forward: kv_split = 2 / kv_f16 = 1)
    def dq_call(fmt, grouped, recompute, probs_tiles=1):
        n_slots = S + 1 if grouped else E
        ds, delta, dq = Canary(E * H * nbT * Tp), Canary(E * H * nbT), Canary(n_slots * dq_stride)
        pr = Canary(E * H * nbT * Tp)
        ids, off, ng = ae._groups(q_idx, S) if grouped else (None, None, 0)
        with _Flags(L, 2, fmt):
            if recompute:
                rc = lib.csn_block_attn_bwd_dq_recompute_f32(
                    dp(fmt), cp(fmt), cstride, qp(fmt), mstride, qi.data_ptr(), k_ptr, v_ptr, kvs, ki.data_ptr(), ld, pr.ptr, ds.ptr,
                    lse.ptr, delta.ptr, dq.ptr, dq_stride, qi.data_ptr() if grouped else None, 0,
                    ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, p, seed, ldp, int(f16), probs_tiles,
                    off.data_ptr() if grouped else None, ng, _stream())
            else:
                rc = lib.csn_block_attn_bwd_dq_f32(
                    dp(fmt), cp(fmt), cstride, k_ptr, v_ptr, kvs, ki.data_ptr(), ld, sc.ptr, ds.ptr, lse.ptr, delta.ptr, dq.ptr,
                    dq_stride, qi.data_ptr() if grouped else None, 0, ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, p,
                    seed, 0, 0, kv_split, ldp, probs_tiles, off.data_ptr() if grouped else None, ng, _stream())
        L.check(rc, "dq")
        pr.check(torch.zeros(pr.n, dtype=torch.bool, device="cuda"), "probs (one plane: unused)")
        return ds, delta, dq

    def dq_form(grouped, recompute, probs_tiles=1):
        what = f"dq{' recompute' if recompute else ''}{' grouped' if grouped else ''}{'' if probs_tiles else ' without planes'}"
        n_slots = S + 1 if grouped else E
        slots = sorted(set(q_idx)) if grouped else range(E)
        ds, delta, dq = dq_call(0, grouped, recompute, probs_tiles)
        delta.check(stat_w, "delta")
        dq.check(a16.map_written(n_slots, slots, dq_stride, D, ld, N, "cuda"), what)
        nothing = torch.zeros(ds.n, dtype=torch.bool, device="cuda")
        ds.check(ae._score_written(r, True, one_plane=True) if probs_tiles else nothing, "[P | dS] planes")
        if ref is not None:
            want = slot_ref("dq", q_idx, n_slots) if grouped else ref["dq"]
            err("dq", maps(dq, n_slots)[list(slots)], want[list(slots)], bb)
            if probs_tiles:
                pv, dv_ = ae._decode_planes(ds, r, which=0), ae._decode_planes(ds, r, which=1)
                ae._pad_zero(pv, r)
                ae._pad_zero(dv_, r)
                err("P", pv[..., :T], ref["P"], fb)
                err("dS", dv_[..., :T], ref["dS"], bb)
        for fmt in fmts:
            ds1, delta1, dq1 = dq_call(fmt, grouped, recompute, probs_tiles)
            _same(delta1, delta, f"delta ({what}, fmt {fmt})")
            _same(ds1, ds, f"[P | dS] planes ({what}, fmt {fmt})")
            if fmt & 4:
                _rounded(dq1, dq, n_slots, slots, dq_stride, D, ld, N, "bf16", f"dQ16 ({what}, fmt {fmt})")
            else:
                _same(dq1, dq, f"dQ ({what}, fmt {fmt})")
        return ds, delta

    def dkv_pair(name, call, grouped):
        """call(fmt) -> (dk, dv) canaries; per evaluation or grouped by key / value slot"""
        n_slots = S + 1 if grouped else E
        slots = sorted(set(kv_idx)) if grouped else range(E)
        dk, dv = call(0)
        w = a16.map_written(n_slots, slots, dq_stride, D, ld, N, "cuda")
        dk.check(w, f"dk ({name})")
        dv.check(w, f"dv ({name})")
        if ref is not None:
            sl = list(slots)
            err("dk", maps(dk, n_slots)[sl], (slot_ref("dk", kv_idx, n_slots) if grouped else ref["dk"])[sl], bb)
            err("dv", maps(dv, n_slots)[sl], (slot_ref("dv", kv_idx, n_slots) if grouped else ref["dv"])[sl], bb)
        for fmt in fmts:
            dk1, dv1 = call(fmt)
            for g1, g0, nm in ((dk1, dk, "dK"), (dv1, dv, "dV")):
                if fmt & 4:
                    _rounded(g1, g0, n_slots, slots, dq_stride, D, ld, N, "bf16", f"{nm}16 ({name}, fmt {fmt})")
                else:
                    _same(g1, g0, f"{nm} ({name}, fmt {fmt})")

    def dkv_call(ds, grouped):
        def call(fmt):
            n_slots = S + 1 if grouped else E
            dk, dv = Canary(n_slots * dq_stride), Canary(n_slots * dq_stride)
            ids, off, ng = ae._groups(kv_idx, S) if grouped else (None, None, 0)
            with _Flags(L, 2, fmt):
                rc = lib.csn_block_attn_bwd_dkv_f32(dp(fmt), cstride, qp(fmt), mstride, qi.data_ptr(), ld, None, ds.ptr, dk.ptr, dv.ptr,
                                                    dq_stride, ki.data_ptr() if grouped else None, ki.data_ptr() if grouped else None,
                                                    0, ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, 0, 0, 0, 0, 1,
                                                    off.data_ptr() if grouped else None, ng, _stream())
            L.check(rc, "dkv")
            return dk, dv
        dkv_pair("products grouped" if grouped else "products", call, grouped)

    def flash_call(delta, grouped):
        def call(fmt):
            n_slots = S + 1 if grouped else E
            dk, dv = Canary(n_slots * dq_stride), Canary(n_slots * dq_stride)
            ids, off, ng = ae._groups(kv_idx, S) if grouped else (None, None, 0)
            with _Flags(L, 2, fmt):
                rc = lib.csn_block_attn_bwd_dkv_flash_f32(
                    dp(fmt), cstride, qp(fmt), mstride, qi.data_ptr(), k_ptr, v_ptr, kvs, ki.data_ptr(), ldp, int(f16), ld, lse.ptr,
                    delta.ptr, dk.ptr, dv.ptr, dq_stride, ki.data_ptr() if grouped else None, ki.data_ptr() if grouped else None, 0,
                    ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, p, seed, off.data_ptr() if grouped else None, ng,
                    _stream())
            L.check(rc, "dkv flash")
            return dk, dv
        dkv_pair("flash grouped" if grouped else "flash", call, grouped)

    ds, delta = dq_form(False, False)
    dq_form(True, False)
    dkv_call(ds, False)
    if "dkv_grouped" in forms:
        dkv_call(ds, True)
    if "dq_recompute" in forms:
        dsr, _ = dq_form(False, True)
        dq_form(True, True)
        _, delta = dq_form(False, True, probs_tiles=0)
        dkv_call(dsr, False)
    if "flash" in forms:
        flash_call(delta, False)
        flash_call(delta, True)
    assert torch.equal(sc.buf, sc_before), "one plane: a dq call touched the kept scores"
    print(f"[act16-edge] {ar.row_id(r)} fwd mode {fwd_mode} fmts {fmts}: bit comparisons so far {_Count.bits}; fp32-map side "
          + " ".join(f"{n} {e:.1e}" for n, e in errs.items()))


IDS2 = [ar.row_id(r) for r in ROWS2]


@pytest.mark.parametrize("r", ROWS2, ids=IDS2)
def test_attention_on_bf16_maps(L, r):
    """Section 1: every mode-2 tile-plane row on bf16 maps (fmt 1, and 5 for the gradient maps) against its fp32-map twin, bits."""
    _attention_row(L, r, 2, (1, 5), ar.row_inputs(r), True)


@pytest.mark.parametrize("r", ROWS2, ids=IDS2)
def test_f16_forward_bf16_backward_on_fp32_maps(L, r):
    """Section 2a: the forward in math mode 3, the backward in mode 2 on the forward's fp16 K / V planes (kv_split = 2, kv_f16 = 1),
    fp32 maps, every output against float64 within BOUNDS[2] — the inputs are exact in fp16 and in bf16 (flush_f16)."""
    _attention_row(L, r, 3, (), a16.flushed_row_inputs(r), True)


@pytest.mark.parametrize("r", ROWS2, ids=IDS2)
def test_f16_forward_bf16_backward_on_16bit_maps(L, r):
    """Section 2b: the same under fmt 2 (backward fmts 2 and 6): Ctx16 = fp16(ctx32), everything else the bits of the fp32-map
    calls fed Ctx16 widened."""
    _attention_row(L, r, 3, (2, 6), a16.flushed_row_inputs(r), False)


# ---- csn_project_f32 writing ONE 16-bit map (out_split = 3), div_rows and a temperature that is no power of two ------------------
@pytest.mark.parametrize("mode,fmt", [(3, "f16"), (2, "bf16")], ids=["mode3-f16", "mode2-bf16"])
@pytest.mark.parametrize("i", range(len(a16.PROJECT16_SHAPES)), ids=[str(s) for s in a16.PROJECT16_SHAPES])
def test_project_writes_one_16bit_map(L, i, mode, fmt):
    """Qs as the forward reads it under the flag: float64 on the rounded operands with ONE rounding of the result to the mode's
    type (bound: tests/act16_ref.py project16_ref); row pitches past the points, NaN there in x, the output in a canary sized for
    the fp32 map."""
    lib = L.lib()
    c = a16.project16_case(i, fmt)
    S, R, C, NP = c["S"], c["R"], c["C"], c["NP"]
    ld_x, ld_o = NP + 4, NP + 8
    xs, os_ = C * ld_x + 16, R * ld_o + 16
    xd = _put32(c["x"], NP, xs, ld_x)
    wd = c["w"].cuda()
    out = Canary(S * os_)
    L.check(lib.csn_set_math_mode(mode))
    L.check(lib.csn_project_f32(xd.data_ptr(), xs, ld_x, wd.data_ptr(), R, C, out.ptr, os_, ld_o, S, NP, c["div_rows"],
                                c["temperature"], 3, 0, _stream()), "csn_project_f32")
    bad = a16.touched16(out.body, a16.map_written16(S, range(S), os_, R, ld_o, NP, "cuda"))
    assert bad == 0, f"{bad} 16-bit elements outside the map were written"
    assert bool((torch.cat((out.buf[:ar.GUARD], out.buf[ar.GUARD + out.n:])) == ar.CANARY32).all())
    got = a16.widen16(_vals16(out, S, os_, R, ld_o, fmt)[..., :NP], fmt)
    ref, bound = a16.project16_ref(c, fmt)
    ratio = a16.ratio(got, ref, bound)
    print(f"[act16-edge] project16 {fmt} {a16.PROJECT16_SHAPES[i]}: error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ---- what the flag refuses (csn_capi.hip): CSN_E_ARG, nothing written, the flag left as it was -----------------------------------
class _Bufs:
    """zero inputs and canary outputs, generous for every call of the table (E = S = H = 1, one block of 32 points, d <= 256)"""

    def __init__(self):
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
        self.map_a, self.map_b, self.map_c = z(256 * 32 * 2), z(256 * 32 * 2), z(256 * 32 * 2)
        self.kv = z(2 * 256 * 1024 * 2, torch.int16)
        self.sc_in, self.stat_in, self.stat_in2 = z(32 * 64), z(64), z(64)
        self.w = z(256 * 256)
        self.ws = z(1 << 16)
        self.out = [Canary(256 * 32 * 2) for _ in range(3)]
        self.sc = [Canary(32 * 64) for _ in range(2)]
        self.stat = [Canary(256) for _ in range(2)]
        self.dw = Canary(256 * 256)

    def untouched(self):
        for c in self.out + self.sc + self.stat + [self.dw]:
            c.check(torch.zeros(c.n, dtype=torch.bool, device="cuda"), "an output of a refused call")


def _p(t):
    return t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr


def _fwd(lib, B, mode, d=32, split=1):
    ldp = 512 * (2 if mode == 1 else 1)
    return lib.csn_block_attn_fwd_f32(_p(B.map_a), _p(B.kv), _p(B.kv) + 2 * d * ldp, d * 32, 2 * d * ldp, None, None, 32, B.out[0].ptr,
                                      d * 32, B.sc[0].ptr, B.stat[0].ptr, 1, 1, d, 32, 1, 32, 8.0, 0.0, 0, split, ldp, _stream())


def _dq(lib, B, mode, d=32, kv_split=1, probs_tiles=1, accumulate=0):
    ldp = 512 * (2 if mode == 1 else 1)
    return lib.csn_block_attn_bwd_dq_f32(_p(B.map_a), _p(B.map_b), d * 32, _p(B.kv), _p(B.kv) + 2 * d * ldp, 2 * d * ldp, None, 32,
                                         B.sc[0].ptr, B.sc[1].ptr, _p(B.stat_in), B.stat[0].ptr, B.out[0].ptr, d * 32, None, accumulate,
                                         None, 1, 1, d, 32, 1, 32, 0.0, 0, 0, 0, kv_split, ldp, probs_tiles, None, 0, _stream())


def _dq_recompute(lib, B, mode, d=32, accumulate=0):
    ldp = 512 * (2 if mode == 1 else 1)
    return lib.csn_block_attn_bwd_dq_recompute_f32(_p(B.map_a), _p(B.map_b), d * 32, _p(B.map_c), d * 32, None, _p(B.kv),
                                                   _p(B.kv) + 2 * d * ldp, 2 * d * ldp, None, 32, B.sc[0].ptr, B.sc[1].ptr,
                                                   _p(B.stat_in), B.stat[0].ptr, B.out[0].ptr, d * 32, None, accumulate, None, 1, 1, d,
                                                   32, 1, 32, 0.0, 0, ldp, 0, 1, None, 0, _stream())


def _dkv(lib, B, mode, d=32, probs_tiles=1, accumulate=0):
    return lib.csn_block_attn_bwd_dkv_f32(_p(B.map_a), d * 32, _p(B.map_b), d * 32, None, 32, _p(B.sc_in), _p(B.sc_in), B.out[0].ptr,
                                          B.out[1].ptr, d * 32, None, None, accumulate, None, 1, 1, d, 32, 1, 32, 0, 0, 0, 0,
                                          probs_tiles, None, 0, _stream())


def _flash(lib, B, mode, d=32, accumulate=0):
    ldp = 512 * (2 if mode == 1 else 1)
    return lib.csn_block_attn_bwd_dkv_flash_f32(_p(B.map_a), d * 32, _p(B.map_b), d * 32, None, _p(B.kv), _p(B.kv) + 2 * d * ldp,
                                                2 * d * ldp, None, ldp, 0, 32, _p(B.stat_in), _p(B.stat_in2), B.out[0].ptr, B.out[1].ptr,
                                                d * 32, None, None, accumulate, None, 1, 1, d, 32, 1, 32, 0.0, 0, None, 0, _stream())


def _dv_scores(lib, B, mode, d=256):
    return lib.csn_block_attn_bwd_dv_scores_f32(_p(B.map_a), d * 32, 32, _p(B.sc_in), _p(B.stat_in), B.out[0].ptr, d * 32, None, None,
                                                1, 1, d, 32, 1, 32, 0.0, 0, None, 0, _stream())


def _oln_fwd(lib, B, mode):
    return lib.csn_outproj_ln_fwd_f32(_p(B.map_a), 32 * 32, _p(B.w), _p(B.map_b), 32 * 32, None, B.out[0].ptr, 32 * 32, B.stat[0].ptr,
                                      1, 32, 32, 32, 32, 1e-6, 0.0, 0, None, None, 0, _stream())


def _oln_bwd(lib, B, mode, dctx_split=0):
    return lib.csn_outproj_ln_bwd_f32(_p(B.map_a), _p(B.map_b), _p(B.stat_in), 32 * 32, _p(B.map_c), 32 * 32, _p(B.w), B.out[0].ptr,
                                      B.out[1].ptr, B.out[2].ptr, B.dw.ptr, _p(B.ws), B.ws.numel(), 1, 32, 32, 32, 32, 0, 0.0, 0,
                                      dctx_split, 32 * 32 if dctx_split else 0, None, 1, None, 1, _stream())


def _cross_fwd(lib, B, mode):
    return lib.csn_cross_attn_fwd_f32(_p(B.map_a), _p(B.map_b), _p(B.map_c), 32 * 32, 32 * 32, 32, 32, B.out[0].ptr, 32 * 32,
                                      B.sc[0].ptr, B.stat[0].ptr, 1, 1, 32, 32, 32, 32, 8.0, 0.0, 0, _stream())


def _cross_bwd(lib, B, mode):
    return lib.csn_cross_attn_bwd_f32(_p(B.map_a), _p(B.map_a), 32 * 32, _p(B.map_a), _p(B.map_b), _p(B.map_c), 32 * 32, 32 * 32, 32, 32,
                                      B.sc[0].ptr, B.sc[1].ptr, _p(B.stat_in), B.stat[0].ptr, B.out[0].ptr, B.out[1].ptr, B.out[2].ptr,
                                      32 * 32, 32 * 32, 1, 1, 32, 32, 32, 32, 0.0, 0, _stream())


def _mix_bwd(lib, B, mode):
    return lib.csn_mix_bwd_f32(_p(B.map_a), _p(B.map_b), _p(B.stat_in), _p(B.stat_in2), B.out[0].ptr, B.stat[0].ptr, B.stat[1].ptr,
                               1, 2, 8, 32, None, None, _stream())


# (id, math mode, fmt, call, control).  control = (math mode, fmt) in which the SAME arguments are taken (the refusal is the flag's
# alone), or None where the call has no accepted twin of the same arguments
REFUSALS = [
    ("fwd-bf16-mode-takes-no-f16-maps", 2, 2, _fwd, (2, 1)),
    ("fwd-f16-mode-takes-no-bf16-maps", 3, 1, _fwd, (3, 2)),
    ("outproj-fwd-bf16-mode-takes-no-f16-maps", 2, 2, _oln_fwd, (2, 1)),
    ("outproj-fwd-f16-mode-takes-no-bf16-maps", 3, 1, _oln_fwd, (3, 2)),
    ("dq-outside-mode-2", 1, 1, _dq, (1, 0)),
    ("dq-recompute-outside-mode-2", 1, 2, _dq_recompute, (1, 0)),
    ("dkv-outside-mode-2", 1, 1, _dkv, (1, 0)),
    ("flash-outside-mode-2", 1, 5, _flash, (1, 0)),
    ("outproj-bwd-outside-mode-2", 1, 2, _oln_bwd, (1, 0)),
    ("cross-length-fwd-block_q", 2, 1, _cross_fwd, (2, 0)),
    ("cross-length-bwd-block_q", 2, 1, _cross_bwd, (2, 0)),
    ("fwd-no-tile-planes", 2, 1, lambda lib, B, m: _fwd(lib, B, m, split=0), None),
    ("dq-no-tile-planes", 2, 1, lambda lib, B, m: _dq(lib, B, m, kv_split=0), None),
    ("dq-probs_tiles-0", 2, 1, lambda lib, B, m: _dq(lib, B, m, probs_tiles=0), None),
    ("dq-probs_tiles-2", 2, 1, lambda lib, B, m: _dq(lib, B, m, probs_tiles=2), None),
    ("dq-probs_tiles-2-where-the-kernel-exists", 1, 1, lambda lib, B, m: _dq(lib, B, m, d=256, probs_tiles=2), (1, 0)),
    ("dkv-probs_tiles-0", 2, 1, lambda lib, B, m: _dkv(lib, B, m, probs_tiles=0), None),
    ("dq-accumulate-fmt5", 2, 5, lambda lib, B, m: _dq(lib, B, m, accumulate=1), (2, 1)),
    ("dq-recompute-accumulate-fmt6", 2, 6, lambda lib, B, m: _dq_recompute(lib, B, m, accumulate=1), (2, 2)),
    ("dkv-accumulate-fmt5", 2, 5, lambda lib, B, m: _dkv(lib, B, m, accumulate=1), (2, 1)),
    ("dkv-accumulate-fmt6", 2, 6, lambda lib, B, m: _dkv(lib, B, m, accumulate=1), (2, 2)),
    ("flash-accumulate-fmt5", 2, 5, lambda lib, B, m: _flash(lib, B, m, accumulate=1), (2, 1)),
    ("flash-accumulate-fmt6", 2, 6, lambda lib, B, m: _flash(lib, B, m, accumulate=1), (2, 2)),
    ("outproj-bwd-dctx_split", 2, 1, lambda lib, B, m: _oln_bwd(lib, B, m, dctx_split=1), None),
    ("dv-from-scores", 1, 1, _dv_scores, (1, 0)),
    ("mix-bwd-with-gradient-maps", 2, 1, _mix_bwd, (2, 0)),
]


@pytest.mark.parametrize("name,mode,fmt,call,control", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_what_the_flag_refuses(L, name, mode, fmt, call, control):
    lib = L.lib()
    B = _Bufs()
    L.check(lib.csn_set_math_mode(mode))
    L.check(lib.csn_set_thread_act16(fmt))
    rc = call(lib, B, mode)
    assert lib.csn_get_thread_act16() == fmt, "a refused call changed the flag"
    L.check(lib.csn_set_thread_act16(0))
    torch.cuda.synchronize()
    assert rc == E_ARG, f"{name}: status {rc}, not CSN_E_ARG"
    B.untouched()
    if control is not None:                               # the same arguments are taken where the header says they are
        cmode, cfmt = control
        L.check(lib.csn_set_math_mode(cmode))
        L.check(lib.csn_set_thread_act16(cfmt))
        rc = call(lib, B, cmode)
        L.check(lib.csn_set_thread_act16(0))
        torch.cuda.synchronize()
        assert rc == 0, f"{name}: the control (mode {cmode}, fmt {cfmt}) returned {rc}"


# ---- out-projection + LayerNorm in math modes 2 and 3: fp32 maps against float64 within DERIVED bounds, 16-bit maps against them, bits
# The edge each shape of a16.OUTPROJ_SHAPES is chosen for:
#   (32, 32, 4, 4) the smallest call;  (32, 36, 60, 64) D % 32 == 4 (k tail of BK = 32), NP % 8 == 4, pitch past the points;
#   (64, 64, 124, 128) one short of BN = 128;  (96, 100, 132, 132) four points past BN;  (128, 128, 68, 72) the LayerNorm backward's
#   64-point group plus four;  (256, 256, 220, 224) the last size of C = 256 on the small kernel;  (256, 256, 224, 224) the first on
#   the 256 x 256 tiles;  (256, 64, 260, 264) ragged second tile, dCtx on the 64-row tile;  (256, 192, 508, 512) dCtx M = 192,
#   N >= 224: big tiles;  (128, 256, 228, 228) small forward kernel, big-tile dCtx.
OUT_IDS = [a16.outproj_id(i) for i in range(len(a16.OUTPROJ_SHAPES))]
E3 = a16.E_OUT
_worst = {}


def _hold(name, got, ref_bound, out):
    r = a16.ratio(got, *ref_bound)
    out[name] = max(out.get(name, 0.0), r)
    _worst[name] = max(_worst.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: error / derived bound = {r:.3f}"


class _OutProj:
    """the buffers and calls of one case (maps of the backward dense: eval stride C ld, as xhat_sum requires of xhat)"""

    def __init__(self, L, c):
        self.L, self.lib, self.c = L, L.lib(), c
        C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
        self.es, self.cs, self.xs = C * ld, D * ld + 16, C * ld + 16
        self.w = c["w"].cuda()
        self.wt = c["w"].t().contiguous().cuda()
        self.x = _put32(c["x"], NP, self.xs)
        self.res = torch.tensor(a16.RES_INDEX, dtype=torch.int32, device="cuda")
        self.ctx32 = _put32(c["ctx"], NP, self.cs)
        self.dxhat = _put32(c["dxhat"], NP, self.es)
        self.rows, self.scale = c["rows"].cuda(), c["scale"].cuda()
        self.xhat_w = a16.map_written(E3, range(E3), self.es, C, ld, NP, "cuda")
        self.dctx_w = a16.map_written(E3, range(E3), self.cs, D, ld, NP, "cuda")
        self.all = lambda n: torch.ones(n, dtype=torch.bool, device="cuda")

    def ctx16(self, fmt):
        return _put16(self.c["ctx"], self.c["NP"], self.cs, fmt)

    def forward(self, mode, fmt, ctx, with_ws):
        c, lib = self.c, self.lib
        C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
        xhat, rstd, sums = Canary(E3 * self.es), Canary(E3 * NP), Canary(E3 * C)
        ws_n = lib.csn_outproj_ln_workspace_floats(E3, C, D, NP) if with_ws else 0
        ws = torch.empty((max(ws_n, 4),), device="cuda")
        with _Flags(self.L, mode, fmt):
            self.L.check(lib.csn_outproj_ln_fwd_f32(ctx.data_ptr(), self.cs, self.w.data_ptr(), self.x.data_ptr(), self.xs,
                                                    self.res.data_ptr(), xhat.ptr, self.es, rstd.ptr, E3, C, D, ld, NP, a16.EPS_LN,
                                                    c["p"], c["seed"], sums.ptr, ws.data_ptr() if with_ws else None, ws_n, _stream()),
                         "csn_outproj_ln_fwd_f32")
        rstd.check(self.all(rstd.n), "rstd")
        sums.check(self.all(sums.n), "xhat_sum")
        return xhat, rstd, sums

    def maps32(self, cn, R, stride):
        c = self.c
        return cn.f32().view(E3, stride)[:, :R * c["ld"]].view(E3, R, c["ld"])[..., :c["NP"]]

    def maps16(self, cn, R, stride, fmt):
        c = self.c
        return a16.widen16(_vals16(cn, E3, stride, R, c["ld"], fmt)[..., :c["NP"]], fmt)

    def backward(self, fmt, form, with_res, xhat_ptr, rstd, ctx_ptr, dz=None, dz_ptr=None):
        c, lib = self.c, self.lib
        C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
        _, n_dense, use_rows, use_scale = form
        dz = dz or Canary(E3 * self.es)
        dzr = Canary(E3 * self.es) if with_res else None
        dctx, dw = Canary(E3 * self.cs), Canary(C * D)
        ws_n = lib.csn_wgrad_workspace_floats(C, D, E3, NP)
        ws = torch.empty((ws_n,), device="cuda")
        with _Flags(self.L, 2, fmt):
            self.L.check(lib.csn_outproj_ln_bwd_f32(self.dxhat.data_ptr(), xhat_ptr, rstd.ptr, self.es, ctx_ptr, self.cs,
                                                    self.wt.data_ptr(), dz_ptr or dz.ptr, dzr.ptr if dzr else None, dctx.ptr, dw.ptr,
                                                    ws.data_ptr(), ws_n, E3, C, D, ld, NP, 0, c["p"], c["seed"], 0, 0,
                                                    self.rows.data_ptr() if use_rows else None, n_dense,
                                                    self.scale.data_ptr() if use_scale else None, 2 if use_scale else 1, _stream()),
                         "csn_outproj_ln_bwd_f32")
        dw.check(self.all(dw.n), "dwfc")
        return dz, dzr, dctx, dw


def _forward_pair(o, mode, tfmt, ffmt, out):
    """part a: the fp32-map forward against float64 (with and without the sums' workspace); part b: the 16-bit forward against it"""
    c = o.c
    ref = a16.outproj_fwd(c)
    fwd = {}
    for with_ws in (True, False):
        xhat, rstd, sums = o.forward(mode, 0, o.ctx32, with_ws)
        xhat.check(o.xhat_w, "xhat")
        _hold("xhat", o.maps32(xhat, c["C"], o.es), ref["xhat"], out)
        _hold("rstd", rstd.f32().view(E3, -1), ref["rstd"], out)
        _hold("xhat_sum" + ("" if with_ws else " (no workspace)"), sums.f32().view(E3, -1), ref["sums"], out)
        fwd[with_ws] = (xhat, rstd, sums)
    assert torch.equal(fwd[True][0].buf, fwd[False][0].buf) and torch.equal(fwd[True][1].buf, fwd[False][1].buf)
    xhat32, rstd32, _ = fwd[True]
    ctx16 = o.ctx16(tfmt)
    for with_ws in (True, False):
        xhat16, rstd16, sums16 = o.forward(mode, ffmt, ctx16, with_ws)
        _same(rstd16, rstd32, "rstd")
        _rounded(xhat16, xhat32, E3, range(E3), o.es, c["C"], c["ld"], c["NP"], "f16", "xhat16")
        xh = o.maps16(xhat16, c["C"], o.es, "f16").double()
        bound = (c["NP"] * a16.U + 2.0 ** -11) * xh.abs().sum(2)           # the rowsum's own bound + one fp16 rounding per term
        _hold("xhat_sum on fp16 maps", sums16.f32().view(E3, -1), (xh.sum(2), bound), out)
    return xhat32, rstd32, xhat16, ctx16


@pytest.mark.parametrize("i", range(len(OUT_IDS)), ids=OUT_IDS)
def test_outproj_ln_mode2(L, i):
    """csn_outproj_ln_fwd_f32 / csn_outproj_ln_bwd_f32 in math mode 2: fp32 maps against float64 within the derived bounds of
    tests/act16_ref.py; bf16 / fp16 maps (fmt 1, and 2 in the backward) against the fp32-map calls fed the same values, bits."""
    c = a16.outproj_case(i, "bf16")
    o = _OutProj(L, c)
    out = {}
    C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
    xhat32, rstd32, xhat16, ctx16 = _forward_pair(o, 2, "bf16", 1, out)
    keep = c["keep"].cuda()
    xh_in = o.maps32(xhat32, C, o.es).double().cpu()
    rs_in = rstd32.f32().view(E3, NP).double().cpu()
    xhat_feed = torch.full((E3, o.es), float("nan"), device="cuda")         # xhat16 widened: what the fp32 side of part b reads
    xhat_feed.view(E3, C, ld)[..., :NP] = o.maps16(xhat16, C, o.es, "f16")
    ctx_f16 = o.ctx16("f16")                                                # the Ctx map of an fp16 forward: the same values
    for form in a16.OUTPROJ_FORMS:
        for with_res in (True, False):
            # part a: the forward's own fp32 xhat
            dz, dzr, dctx, dw = o.backward(0, form, with_res, xhat32.ptr, rstd32, o.ctx32.data_ptr())
            dz.check(o.xhat_w, "dz")
            dctx.check(o.dctx_w, "dctx")
            ln = a16.outproj_ln_bwd(c, form, xh_in, rs_in)
            dzv = o.maps32(dz, C, o.es)
            assert bool((dzv[~keep] == 0).all()), "dz: a dropped element is not an exact zero"
            _hold("dz", dzv, ln["dz"], out)                                  # (dropped elements: 0 against 0 +- 0)
            if with_res:
                dzr.check(o.xhat_w, "dz_res")
                _hold("dz_res", o.maps32(dzr, C, o.es), ln["dz_res"], out)    # no mask in it
            pr = a16.outproj_products(c, dzv.cpu())
            _hold("dctx", o.maps32(dctx, D, o.cs), pr["dctx"], out)
            _hold("dwfc", dw.f32().view(C, D), pr["dwfc"], out)
            # part b: xhat16 and Ctx16 against the fp32-map call fed both widened
            dz0, dzr0, dctx0, dw0 = o.backward(0, form, with_res, xhat_feed.data_ptr(), rstd32, o.ctx32.data_ptr())
            for fmt, cx in ((1, ctx16), (2, ctx_f16)):
                dz1, dzr1, dctx1, dw1 = o.backward(fmt, form, with_res, xhat16.ptr, rstd32, cx.data_ptr())
                _rounded(dz1, dz0, E3, range(E3), o.es, C, ld, NP, "bf16", f"dz16 (fmt {fmt})")
                _rounded(dctx1, dctx0, E3, range(E3), o.cs, D, ld, NP, "bf16", f"dCtx16 (fmt {fmt})")
                _same(dw1, dw0, f"dW_fc (fmt {fmt})")
                if with_res:
                    _same(dzr1, dzr0, f"dz_res (fmt {fmt})")
                z1 = a16.widen16(_vals16(dz1, E3, o.es, C, ld, "bf16")[..., :NP], "bf16") == 0
                assert torch.equal(z1, o.maps32(dz0, C, o.es) == 0) and bool(z1[~keep].all()), "the dropout zeros differ"
    print(f"[act16-edge] outproj mode 2 {OUT_IDS[i]}: error / bound " + " ".join(f"{n} {r:.3f}" for n, r in out.items())
          + f"; bit comparisons so far {_Count.bits}")


@pytest.mark.parametrize("i", range(len(OUT_IDS)), ids=OUT_IDS)
def test_outproj_ln_fwd_mode3(L, i):
    """the forward in math mode 3 (fp16 operands): fp32 maps against float64, fp16 maps (fmt 2) against them"""
    o = _OutProj(L, a16.outproj_case(i, "f16"))
    out = {}
    _forward_pair(o, 3, "f16", 2, out)
    print(f"[act16-edge] outproj mode 3 {OUT_IDS[i]}: error / bound " + " ".join(f"{n} {r:.3f}" for n, r in out.items())
          + f"; bit comparisons so far {_Count.bits}")


def test_outproj_16bit_maps_at_the_end_of_their_allocation(L):
    """tests/test_gpu_act16.py's allocation-end layout for Ctx16 (read by the forward, the delta-free W_fc gradient) and for dz16
    (written by the LayerNorm backward, read as the k-contiguous operand of dCtx and of the W_fc gradient): each map ends exactly
    where a guard of 16-bit NaN begins, NP % 8 == 4 (the last 16-byte unit of every row straddles the end of the row).  The
    results are finite, the bits of the fp32-map calls, and the guards untouched."""
    i = 9                                                                   # (128, 256, 228, 228): ld == NP, big-tile dCtx
    c = a16.outproj_case(i, "bf16")
    o = _OutProj(L, c)
    C, D, NP, ld = (c[n] for n in ("C", "D", "NP", "ld"))
    assert ld == NP and NP % 8 == 4
    o.cs = D * ld                                                           # dense: the last evaluation's last row ends the map
    o.dctx_w = a16.map_written(E3, range(E3), o.cs, D, ld, NP, "cuda")
    o.ctx32 = _put32(c["ctx"], NP, o.cs)
    nan = a16.nan16("bf16")
    n_ctx, n_dz, guard = E3 * D * ld, E3 * C * ld, 4096
    pool_c = torch.full((n_ctx + guard,), nan, dtype=torch.int16, device="cuda")
    pool_c[:n_ctx].view(E3, D, ld).copy_(a16.bits16(c["ctx"].cuda(), "bf16"))
    pool_z = torch.full((n_dz + guard,), nan, dtype=torch.int16, device="cuda")
    ctx16 = pool_c[:n_ctx]
    assert ctx16.data_ptr() + 2 * n_ctx == pool_c[n_ctx:].data_ptr()
    xhat32, rstd32, _ = o.forward(2, 0, o.ctx32, False)
    xhat16, rstd16, _ = o.forward(2, 1, ctx16, False)
    _same(rstd16, rstd32, "rstd")
    _rounded(xhat16, xhat32, E3, range(E3), o.es, C, ld, NP, "f16", "xhat16")
    xhat_feed = torch.full((E3, o.es), float("nan"), device="cuda")
    xhat_feed.view(E3, C, ld)[..., :NP] = o.maps16(xhat16, C, o.es, "f16")
    form = a16.OUTPROJ_FORMS[0]
    dz0, dzr0, dctx0, dw0 = o.backward(0, form, True, xhat_feed.data_ptr(), rstd32, o.ctx32.data_ptr())
    _, dzr1, dctx1, dw1 = o.backward(1, form, True, xhat16.ptr, rstd32, ctx16.data_ptr(), dz=Canary(4), dz_ptr=pool_z.data_ptr())
    torch.cuda.synchronize()
    assert bool((pool_c[n_ctx:] == nan).all()) and bool((pool_z[n_dz:] == nan).all()), "a guard was written"
    assert bool(torch.isfinite(dw1.f32()).all()) and bool(torch.isfinite(o.maps16(dctx1, D, o.cs, "bf16")).all())
    _same(dw1, dw0, "dW_fc")
    _same(dzr1, dzr0, "dz_res")
    _rounded(dctx1, dctx0, E3, range(E3), o.cs, D, ld, NP, "bf16", "dCtx16")
    assert torch.equal(pool_z[:n_dz].view(E3, C, ld), a16.bits16(o.maps32(dz0, C, o.es), "bf16")), "dz16 is not bf16(dz32)"
    print(f"[act16-edge] allocation end: bit comparisons so far {_Count.bits}")
