"""Every block-attention kernel instance at the edges of its key tiles, through the raw C ABI, against the float64 reference of
tests/attn_edge_ref.py: blocks shorter than one 32-key tile, whole tiles, one partial tile past whole ones, a short last block
(ld ending inside it), live dropout, a score pitch past the round-up of the block, tile-major scores.  The probe rows of the
inputs turn a one-key error (a key lost, a padding key let in, the mask shifted) into an error 10x the mode's bound
(tests/test_cpu_attn_edges.py shows that without a GPU).  Every output lies inside a larger buffer filled with a NaN pattern:
the guards and every element the contract leaves alone must keep it; K / V tile planes hold NaN in the tiles past a block's
last one ("never read", include/csn_hip.h)."""
import numpy as np
import pytest
import torch

from tests import attn_edge_ref as ar

pytestmark = pytest.mark.gpu

ROWS = ar.rows()
Canary = ar.Canary


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_thread_score_layout(0)
    L.lib().csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _map_written(n_slots, slots, stride, D, ld, N):
    m = torch.zeros((n_slots, stride), dtype=torch.bool, device="cuda")
    for s in slots:
        m[s, :D * ld].view(D, ld)[:, :N] = True
    return m


def _stat_written(E, H, nbT, N):
    m = torch.zeros((E, H, nbT), dtype=torch.bool, device="cuda")
    m[..., :N] = True
    return m


def _score_written(r, full_tiles, tile_major=False, one_plane=False):
    """region of a scores / P / dS buffer [E][H][nb][T][Tp] floats that a call writes: rows < T_b and keys < T_b (fp32 scores)
    or every key of the tiles < round-up-32(T_b) / 32 (tile planes: their padding keys are written as zeros).  one_plane: the
    mode-2 [P rows | dS rows] region of bf16 rows of pitch Tp (int32 units: pitch Tp / 2)."""
    E, H, nb, T, Tp = r["E"], r["H"], r["nb"], r["T"], r["Tp"]
    m = torch.zeros((E, H, nb, T * Tp), dtype=torch.bool, device="cuda")
    for b, Tb in enumerate(ar.block_lengths(T, nb, r["T_last"])):
        nk = ar.ceil_to(Tb, ar.KT) if full_tiles else Tb
        if one_plane:
            v = m[:, :, b].view(E, H, 2, T, Tp // 2)
            v[:, :, :, :Tb, :nk // 2] = True
        elif tile_major:
            v = m[:, :, b].view(E, H, Tp // ar.KT, T, ar.KT)
            for kt in range(ar.ceil_to(Tb, ar.KT) // ar.KT):
                v[:, :, kt, :Tb, :max(0, min(ar.KT, nk - kt * ar.KT))] = True
        else:
            m[:, :, b].view(E, H, T, Tp)[:, :, :Tb, :nk] = True
    return m


def _decode_scores(buf, r, tile_major=False):
    """fp32 scores [E][H][nb][T][Tp] (row-major or tile-major) -> (E, H, nb, T, Tp) [query][key]"""
    E, H, nb, T, Tp = r["E"], r["H"], r["nb"], r["T"], r["Tp"]
    x = buf.f32().view(E, H, nb, -1)
    if tile_major:
        return x.view(E, H, nb, Tp // 32, T, 32).permute(0, 1, 2, 4, 3, 5).reshape(E, H, nb, T, Tp)
    return x.view(E, H, nb, T, Tp)


def _decode_planes(buf, r, tile_major=False, which=0):
    """tile planes of P / dS -> values (E, H, nb, T, Tp).  Mode 1: per query row 16 tiles [hi 32 | lo 32] bf16 (the bytes of the
    fp32 row; tile-major: [tile][query][64]); mode 2: [P rows | dS rows] (which = 0 / 1) of Tp bf16 elements."""
    E, H, nb, T, Tp = r["E"], r["H"], r["nb"], r["T"], r["Tp"]
    x = buf.body.view(torch.bfloat16).view(E, H, nb, -1)
    if r["mode"] == 2:
        return x.view(E, H, nb, 2, T, Tp)[:, :, :, which].float()
    if tile_major:
        x = x.view(E, H, nb, Tp // 32, T, 2, 32).permute(0, 1, 2, 4, 3, 5, 6)
    else:
        x = x.view(E, H, nb, T, Tp // 32, 2, 32)
    return (x[..., 0, :].float() + x[..., 1, :].float()).reshape(E, H, nb, T, Tp)


def _pad_zero(vals, r):
    """the padding keys T_b .. round-up-32(T_b) of every written row hold exact zeros"""
    for b, Tb in enumerate(ar.block_lengths(r["T"], r["nb"], r["T_last"])):
        pad = vals[:, :, b, :Tb, Tb:ar.ceil_to(Tb, ar.KT)]
        if pad.numel():
            assert bool((pad == 0).all()), "tile-plane padding keys are not zero"


def _groups(idx, n_slots):
    """eval_ids / group_offsets grouping the evaluations by slot (adjacent), as device int32 arrays"""
    idx = np.asarray(idx)
    order = np.argsort(idx, kind="stable").astype(np.int32)
    off = [0]
    for s in range(n_slots):
        c = int((idx == s).sum())
        if c:
            off.append(off[-1] + c)
    return (torch.from_numpy(order).cuda(), torch.tensor(off, dtype=torch.int32, device="cuda"), len(off) - 1)


def _colours(idx):
    """evaluations split into colours in which no two share a slot (first occurrence first)"""
    seen, cols = {}, []
    for e, s in enumerate(idx):
        c = seen.get(s, 0)
        seen[s] = c + 1
        while len(cols) <= c:
            cols.append([])
        cols[c].append(e)
    return [torch.tensor(c, dtype=torch.int32, device="cuda") for c in cols]


@pytest.mark.parametrize("r", ROWS, ids=[ar.row_id(r) for r in ROWS])
def test_attention_edges(L, r):
    lib = L.lib()
    mode, tp = r["mode"], r["kv"] == "tp"
    L.check(lib.csn_set_math_mode(mode))
    S, E, H, d, T, nb, Tl, Tp, p, seed = (r[n] for n in ("S", "E", "H", "d", "T", "nb", "T_last", "Tp", "p", "seed"))
    assert lib.csn_attn_bwd_grouping(d, T) == ar.grouping(mode, d, T)
    forms = ar.forms(r)
    D, N = H * d, ar.n_points(T, nb, Tl)
    ld = N + r["pad"]
    nbT = nb * T
    fb, bb = ar.BOUNDS[mode]
    q, k, v, dctx = ar.row_inputs(r)
    q_idx, kv_idx = r["q_idx"], r["kv_idx"]
    qi = torch.tensor(q_idx, dtype=torch.int32, device="cuda")
    ki = torch.tensor(kv_idx, dtype=torch.int32, device="cuda")

    # ---- inputs: fp32 maps with NaN past the last point and between slots; K / V tile planes with NaN tiles past each block's last
    mstride = D * ld + 16

    def put_map(x):
        buf = torch.full((x.shape[0], mstride), float("nan"), device="cuda")
        buf[:, :D * ld].view(-1, D, ld)[..., :N] = x[..., :N].cuda()
        return buf

    qd, dd = put_map(q), put_map(dctx)
    npl = 2 if mode == 1 else 1
    if tp:
        ldp = nb * ar.BLOCK_PITCH * npl
        planes = ar.pack_tile_planes(torch.cat((k, v), 1), T, nb, npl, "f16" if mode == 3 else "bf16", Tl)
        kvs = 2 * D * ldp + 64
        kvbuf = torch.full((S, kvs), ar.NAN_BF16, dtype=torch.int16, device="cuda")
        kvbuf[:, :2 * D * ldp] = planes.reshape(S, -1).cuda()
        k_ptr, v_ptr, split = kvbuf.data_ptr(), kvbuf.data_ptr() + 2 * D * ldp, 1
    else:
        ldp, kvs = 0, mstride
        kd, vd = put_map(k), put_map(v)
        k_ptr, v_ptr, split = kd.data_ptr(), vd.data_ptr(), 0

    # ---- float64 reference (slots gathered per evaluation)
    keep, _ = ar.row_masks(r)
    ref = ar.block_attention_ref(*(ar.per_eval(t, ix, H).cuda() for t, ix in ((q, q_idx), (k, kv_idx), (v, kv_idx))),
                                 dctx.double().view(E, H, d, ld).cuda(), T, nb, Tl, keep, p)
    errs = {}

    def err(name, got, want, bound):
        e = ar.per_block_err(got, want, T, nb, Tl)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e < bound, f"{name}: per-block error {e:.3e} >= {bound:.1e}"

    cstride = mstride                          # (one ctx_eval_stride for ctx and dctx)
    ctx_w = _map_written(E, range(E), cstride, D, ld, N)
    stat_w = _stat_written(E, H, nbT, N)
    maps = lambda c, n: c.f32().view(n, -1)[:, :D * ld].view(n, H, d, ld)

    # ---- forward: with and without kept scores (bitwise the same), repeatable, another seed moves the dropped rows
    def forward(keep_scores, sd=seed, layout=0):
        ctx, lse = Canary(E * cstride), Canary(E * H * nbT)
        sc = Canary(E * H * nbT * Tp) if keep_scores else None
        L.check(lib.csn_set_thread_score_layout(layout))
        rc = lib.csn_block_attn_fwd_f32(qd.data_ptr(), k_ptr, v_ptr, mstride, kvs, qi.data_ptr(), ki.data_ptr(), ld, ctx.ptr,
                                        cstride, sc.ptr if sc else None, lse.ptr, E, H, d, T, nb, Tp, 8.0, p, sd, split, ldp,
                                        _stream())
        L.check(lib.csn_set_thread_score_layout(0))
        L.check(rc, "forward")
        return ctx, lse, sc

    ctx, lse, sc = forward(True)
    ctx.check(ctx_w, "ctx")
    lse.check(stat_w, "lse")
    sc.check(_score_written(r, False), "scores")
    err("ctx", maps(ctx, E), ref["ctx"], fb)
    err("lse", lse.f32().view(E, H, nbT), ref["lse"], fb)
    err("S", _decode_scores(sc, r)[..., :T], ref["S"], fb)
    ctx1, lse1, _ = forward(False)
    assert torch.equal(ctx1.buf, ctx.buf) and torch.equal(lse1.buf, lse.buf), "forward differs without kept scores"
    ctx2, _, sc2 = forward(True)
    assert torch.equal(ctx2.buf, ctx.buf) and torch.equal(sc2.buf, sc.buf), "forward not repeatable"
    if p > 0:
        ctx3, _, _ = forward(False, seed ^ 0x5555)
        assert not torch.equal(ctx3.buf, ctx.buf), "another seed gives the same dropped rows"
    if mode == 3:
        _report(r, errs)
        return

    # ---- backward
    dq_stride = mstride
    lse_p = lse.ptr
    ref_ds_pd = {"P": ref["P"], "dS": ref["dS"]}

    def slot_ref(name, idx, n_slots):
        out = torch.zeros((n_slots, H, d, ld), dtype=torch.float64, device="cuda")
        return out.index_add_(0, torch.tensor(idx, device="cuda"), ref[name])

    def dq_call(kept_sc, probs_tiles, grouped=False, recompute=False, probs=None, layout=0):
        """one dQ call; returns (scores buffer after it, dscores, delta, dq buffer, written slots)"""
        n_slots = S + 1 if grouped else E
        scb = kept_sc.clone() if kept_sc is not None else probs
        ds, delta, dq = Canary(E * H * nbT * Tp), Canary(E * H * nbT), Canary(n_slots * dq_stride)
        ids, off, ng = _groups(q_idx, S) if grouped else (None, None, 0)
        L.check(lib.csn_set_thread_score_layout(layout))
        if recompute:
            rc = lib.csn_block_attn_bwd_dq_recompute_f32(
                dd.data_ptr(), ctx.ptr, cstride, qd.data_ptr(), mstride, qi.data_ptr(), k_ptr, v_ptr, kvs, ki.data_ptr(), ld,
                scb.ptr, ds.ptr, lse_p, delta.ptr, dq.ptr, dq_stride, qi.data_ptr() if grouped else None, 0,
                ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, p, seed, ldp, 0, probs_tiles,
                off.data_ptr() if grouped else None, ng, _stream())
        else:
            rc = lib.csn_block_attn_bwd_dq_f32(
                dd.data_ptr(), ctx.ptr, cstride, k_ptr, v_ptr, kvs, ki.data_ptr(), ld, scb.ptr, ds.ptr, lse_p, delta.ptr, dq.ptr,
                dq_stride, qi.data_ptr() if grouped else None, 0, ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, p,
                seed, 0, 0, split, ldp, probs_tiles, off.data_ptr() if grouped else None, ng, _stream())
        L.check(lib.csn_set_thread_score_layout(0))
        L.check(rc, "dq")
        delta.check(stat_w, "delta")
        slots = sorted(set(q_idx)) if grouped else range(E)
        dq.check(_map_written(n_slots, slots, dq_stride, D, ld, N), "dq")
        want = slot_ref("dq", q_idx, n_slots) if grouped else ref["dq"]
        err("dq", maps(dq, n_slots)[list(slots)], want[list(slots)], bb)
        return scb, ds, delta, dq

    def check_p_ds(scb, ds, tiles, layout=0):
        if not tiles:
            scb.check(_score_written(r, False), "P (fp32 scores)")
            ds.check(_score_written(r, False), "dS (fp32 scores)")
            err("P", _decode_scores(scb, r)[..., :T], ref_ds_pd["P"], fb)
            err("dS", _decode_scores(ds, r)[..., :T], ref_ds_pd["dS"], bb)
            return
        if mode == 2:
            ds.check(_score_written(r, True, one_plane=True), "[P | dS] planes")
            pv, dv_ = _decode_planes(ds, r, which=0), _decode_planes(ds, r, which=1)
        else:
            scb.check(_score_written(r, True, tile_major=layout == 1), "P planes")
            ds.check(_score_written(r, True, tile_major=layout == 1), "dS planes")
            pv, dv_ = _decode_planes(scb, r, layout == 1), _decode_planes(ds, r, layout == 1)
        _pad_zero(pv, r)
        _pad_zero(dv_, r)
        err("P", pv[..., :T], ref_ds_pd["P"], fb)
        err("dS", dv_[..., :T], ref_ds_pd["dS"], bb)

    def dkv_check(dk, dv, n_slots, slots, idx, what):
        w = _map_written(n_slots, slots, dq_stride, D, ld, N)
        dk.check(w, f"dk ({what})")
        dv.check(w, f"dv ({what})")
        sl = list(slots)
        rk = slot_ref("dk", idx, n_slots) if n_slots != E or what != "per evaluation" else ref["dk"]
        rv = slot_ref("dv", idx, n_slots) if n_slots != E or what != "per evaluation" else ref["dv"]
        err("dk", maps(dk, n_slots)[sl], rk[sl], bb)
        err("dv", maps(dv, n_slots)[sl], rv[sl], bb)

    def dkv_call(scb, ds, tiles, grouped=False, layout=0):
        n_slots = S + 1 if grouped else E
        dk, dv = Canary(n_slots * dq_stride), Canary(n_slots * dq_stride)
        ids, off, ng = _groups(kv_idx, S) if grouped else (None, None, 0)
        L.check(lib.csn_set_thread_score_layout(layout))
        rc = lib.csn_block_attn_bwd_dkv_f32(dd.data_ptr(), cstride, qd.data_ptr(), mstride, qi.data_ptr(), ld,
                                            None if (tiles and mode == 2) else scb.ptr, ds.ptr, dk.ptr, dv.ptr, dq_stride,
                                            ki.data_ptr() if grouped else None, ki.data_ptr() if grouped else None, 0,
                                            ids.data_ptr() if grouped else None, E, H, d, T, nb, Tp, 0, 0, 0, 0, int(tiles),
                                            off.data_ptr() if grouped else None, ng, _stream())
        L.check(lib.csn_set_thread_score_layout(0))
        L.check(rc, "dkv")
        dkv_check(dk, dv, n_slots, sorted(set(kv_idx)) if grouped else range(E), kv_idx,
                  "grouped" if grouped else "per evaluation")
        return dk, dv

    if not tp:                                                            # fp32 K / V maps: P / dS as fp32 scores
        scb, ds, delta, dq = dq_call(sc, 0)
        check_p_ds(scb, ds, False)
        again = dq_call(sc, 0)[3]
        assert torch.equal(again.buf, dq.buf), "dq not repeatable"
        dkv_call(scb, ds, False)
        _report(r, errs)
        return

    sc_before = sc.buf.clone()
    scb, ds, delta, dq = dq_call(sc, 1)
    if mode == 2:                                                         # one plane: the scores are left alone
        assert torch.equal(scb.buf, sc_before)
    check_p_ds(scb, ds, True)
    gdq = dq_call(sc, 1, grouped=True)[3]
    dkv_call(scb, ds, True)
    if "dkv_grouped" in forms:
        dkv_call(scb, ds, True, grouped=True)
    delta_rc = delta
    if "dq_recompute" in forms:
        pr = Canary(E * H * nbT * Tp)
        scr, dsr, _, dqr = dq_call(None, 1, recompute=True, probs=pr)
        if mode == 2:
            pr.check(torch.zeros(pr.n, dtype=torch.bool, device="cuda"), "probs (one plane: unused)")
        check_p_ds(scr, dsr, True)
        dkv_call(scr, dsr, True)
        pr0 = Canary(E * H * nbT * Tp)
        scr0, dsr0, delta_rc, dqr0 = dq_call(None, 0, recompute=True, probs=pr0)
        nothing = torch.zeros(pr0.n, dtype=torch.bool, device="cuda")
        scr0.check(nothing, "probs (probs_tiles = 0)")
        dsr0.check(nothing, "dscores (probs_tiles = 0)")
        assert torch.equal(dqr0.buf, dqr.buf), "dq recompute: with and without the planes"
        assert torch.equal(delta_rc.buf, delta.buf), "delta: the recomputing call differs from the kept-scores call"
        again = dq_call(None, 0, recompute=True, probs=Canary(E * H * nbT * Tp))[3]
        assert torch.equal(again.buf, dqr0.buf), "dq recompute not repeatable"
        dq_call(None, 0, grouped=True, recompute=True, probs=Canary(E * H * nbT * Tp))
    if "flash" in forms:
        def flash(n_slots, idx_ptrs, ids, n_launch, off, ng, accumulate=0, dk=None, dv=None):
            dk = dk or Canary(n_slots * dq_stride)
            dv = dv or Canary(n_slots * dq_stride)
            L.check(lib.csn_block_attn_bwd_dkv_flash_f32(
                dd.data_ptr(), cstride, qd.data_ptr(), mstride, qi.data_ptr(), k_ptr, v_ptr, kvs, ki.data_ptr(), ldp, 0, ld, lse_p,
                delta_rc.ptr, dk.ptr, dv.ptr, dq_stride, idx_ptrs, idx_ptrs, accumulate, ids, n_launch, H, d, T, nb, Tp, p, seed,
                off, ng, _stream()), "dkv flash")
            return dk, dv
        fk, fv = flash(E, None, None, E, None, 0)
        dkv_check(fk, fv, E, range(E), kv_idx, "per evaluation")
        fk2, fv2 = flash(E, None, None, E, None, 0)
        assert torch.equal(fk2.buf, fk.buf) and torch.equal(fv2.buf, fv.buf), "dkv flash not repeatable"
        ids, off, ng = _groups(kv_idx, S)
        gk, gv = flash(S + 1, ki.data_ptr(), ids.data_ptr(), E, off.data_ptr(), ng)
        used = sorted(set(kv_idx))
        dkv_check(gk, gv, S + 1, used, kv_idx, "grouped")
        ck, cv = None, None
        for c, ev in enumerate(_colours(kv_idx)):
            ck, cv = flash(S + 1, ki.data_ptr(), ev.data_ptr(), ev.numel(), None, 0, int(c > 0), ck, cv)
        dkv_check(ck, cv, S + 1, used, kv_idx, "colour by colour")
    if "tile_major" in forms:
        ctx_t, lse_t, sc_t = forward(True, layout=1)
        assert torch.equal(ctx_t.buf, ctx.buf) and torch.equal(lse_t.buf, lse.buf)
        sc_t.check(_score_written(r, False, tile_major=True), "tile-major scores")
        bits = lambda x: x.contiguous().view(torch.int32)                 # (elements never written: the same NaN pattern)
        assert torch.equal(bits(_decode_scores(sc_t, r, True)), bits(_decode_scores(sc, r))), "tile-major scores differ"
        scb_t, ds_t, _, dq_t = dq_call(sc_t, 1, layout=1)
        assert torch.equal(dq_t.buf, dq.buf), "tile-major dq differs"
        check_p_ds(scb_t, ds_t, True, layout=1)
        dkv_call(scb_t, ds_t, True, layout=1)
        if "dkv_grouped" in forms:
            dkv_call(scb_t, ds_t, True, grouped=True, layout=1)
    del gdq
    _report(r, errs)


def _report(r, errs):
    print(f"[attn-edge] {ar.row_id(r)}: " + " ".join(f"{n} {e:.1e}" for n, e in errs.items()))
