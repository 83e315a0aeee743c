"""dV from the kept scores (csn_block_attn_bwd_dv_scores_f32) and the three-call backward around it, through the raw C ABI at
d = 256 in math mode 1: the dQ call with probs_tiles = 2 (dS planes only, scores untouched), the dV kernel, the dK-only plane
product — against the current two-call flow (bit for bit where the arithmetic is the same) and, for dV, against the float64
reference of tests/attn_edge_ref.py with the masks of tests/dropout_ref.py.

Blocks: less than one 128-key chunk with a ragged 32-query tile (36), exactly one chunk (128), one 16-key group past a chunk
(132), the production block (500), each with one block and with three; a row that ends inside its last block (block 100,
n_blocks 3, ld 232).  The block-500 cases run in both score layouts (row-major and
tile-major; the tile-major layout exists only where the plane products run on the 256 x 256 tiles).  Four evaluations on key / value slots (0, 0, 1, 2) — one group of two, as csa_train has — whose query
slots (0, 1, 1, 2) differ from the key slot for one of them.

dV bound: both routes are the same three bf16 products of the same operands, P rounded to hi + lo the same way; only the order
in which fp32 partial sums are added differs — so the new kernel may not be worse than twice the plane route on the same inputs,
and stays inside the bound the edge sweep applies to dV (attn_edge_ref.BOUNDS[1]).

Then the module: a CrossShapeAt train-mode step with tuning.dv_from_scores on against off."""
import numpy as np
import pytest
import torch

from tests import attn_edge_ref as ar

pytestmark = pytest.mark.gpu

D_HEAD = 256
Q_IDX, KV_IDX = (0, 1, 1, 2), (0, 0, 1, 2)
GEOMETRIES = [(36, 1, None), (36, 3, None), (128, 1, None), (128, 3, None), (132, 1, None), (132, 3, None),
              (500, 1, None), (500, 3, None), (100, 3, 32), (500, 2, 100)]        # (block, n_blocks, short last block)


def _cases():
    out = []
    for i, (T, nb, Tl) in enumerate(GEOMETRIES):
        for p in (0.0, 0.1):
            for Tp in sorted({ar.ceil_to(T, 32), 512}):
                # tile-major scores exist where the plane products run on the big tiles (block 500 here): both layouts there
                for layout in ((0, 1) if ar.grouping(1, D_HEAD, T) & 16 else (0,)):
                    out.append(dict(mode=1, kv="tp", d=D_HEAD, H=1, T=T, nb=nb, T_last=Tl, p=p, Tp=Tp, pad=0, layout=layout,
                                    seed=(ar.HIGH_SEED + i) if i % 2 else 1000 + 7 * i, S=3, E=4, q_idx=Q_IDX, kv_idx=KV_IDX))
    return out


def _case_id(r):
    return ar.row_id(r) + ("-tilemajor" if r["layout"] else "")


CASES = _cases()


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


def _groups(idx, n_slots):
    idx = np.asarray(idx)
    order = np.argsort(idx, kind="stable").astype(np.int32)
    off = [0]
    for s in range(n_slots):
        c = int((idx == s).sum())
        if c:
            off.append(off[-1] + c)
    return torch.from_numpy(order).cuda(), torch.tensor(off, dtype=torch.int32, device="cuda"), len(off) - 1


def _colours(idx):
    seen, cols = {}, []
    for e, s in enumerate(idx):
        c = seen.get(s, 0)
        seen[s] = c + 1
        while len(cols) <= c:
            cols.append([])
        cols[c].append(e)
    return [torch.tensor(c, dtype=torch.int32, device="cuda") for c in cols]


_inputs = {}


def _row_data(r):
    """inputs and the float64 dV reference of a case's geometry; shared by the cases that differ only in pitch (the reference
    depends on the pitch through the masks alone, so it is kept per (geometry, p, pitch) and the inputs per geometry)"""
    key = (r["T"], r["nb"], r["T_last"])
    if key not in _inputs:
        _inputs[key] = ar.row_inputs(r)
    return _inputs[key]


@pytest.mark.parametrize("r", CASES, ids=[_case_id(r) for r in CASES])
def test_dv_from_scores(L, r):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    S, E, H, d, T, nb, Tl, Tp, p, seed = (r[n] for n in ("S", "E", "H", "d", "T", "nb", "T_last", "Tp", "p", "seed"))
    assert lib.csn_attn_bwd_dv_scores_available(d, T)
    L.check(lib.csn_set_thread_score_layout(r["layout"]))               # every call of the case in the case's score layout
    D, N = H * d, ar.n_points(T, nb, Tl)
    ld, nbT = N, nb * T
    Canary = ar.Canary
    q, k, v, dctx = _row_data(r)
    qi = torch.tensor(Q_IDX, dtype=torch.int32, device="cuda")
    ki = torch.tensor(KV_IDX, dtype=torch.int32, device="cuda")
    mstride = D * ld + 16

    def put_map(x):
        buf = torch.full((x.shape[0], mstride), float("nan"), device="cuda")
        buf[:, :D * ld].view(-1, D, ld)[..., :N] = x[..., :N].cuda()
        return buf

    qd, dd = put_map(q), put_map(dctx)
    ldp = nb * ar.BLOCK_PITCH * 2
    planes = ar.pack_tile_planes(torch.cat((k, v), 1), T, nb, 2, "bf16", Tl)
    kvs = 2 * D * ldp + 64
    kvbuf = torch.full((S, kvs), ar.NAN_BF16, dtype=torch.int16, device="cuda")
    kvbuf[:, :2 * D * ldp] = planes.reshape(S, -1).cuda()
    k_ptr, v_ptr = kvbuf.data_ptr(), kvbuf.data_ptr() + 2 * D * ldp

    # ---- the project's own forward: ctx, lse, kept scores
    ctx, lse, sc = Canary(E * mstride), Canary(E * H * nbT), Canary(E * H * nbT * Tp)
    L.check(lib.csn_block_attn_fwd_f32(qd.data_ptr(), k_ptr, v_ptr, mstride, kvs, qi.data_ptr(), ki.data_ptr(), ld, ctx.ptr, mstride,
                                       sc.ptr, lse.ptr, E, H, d, T, nb, Tp, 8.0, p, seed, 1, ldp, _stream()), "forward")

    n_slots = S + 1
    q_ids, q_off, q_ng = _groups(Q_IDX, S)
    kv_ids, kv_off, kv_ng = _groups(KV_IDX, S)
    grouped_dkv = bool(lib.csn_attn_bwd_grouping(d, T) & 2)

    def dq_call(probs_tiles):
        scb = sc.clone()
        ds, delta, dq = Canary(E * H * nbT * Tp), Canary(E * H * nbT), Canary(n_slots * mstride)
        L.check(lib.csn_block_attn_bwd_dq_f32(dd.data_ptr(), ctx.ptr, mstride, k_ptr, v_ptr, kvs, ki.data_ptr(), ld, scb.ptr, ds.ptr,
                                              lse.ptr, delta.ptr, dq.ptr, mstride, qi.data_ptr(), 0, q_ids.data_ptr(), E, H, d, T, nb,
                                              Tp, p, seed, 0, 0, 1, ldp, probs_tiles, q_off.data_ptr(), q_ng, _stream()), "dq")
        return scb, ds, delta, dq

    def dkv_call(scb, ds, dk, dv):
        """the plane products: grouped where the library offers it, colour by colour elsewhere; scb / dv None: dK alone"""
        def call(ids, n, off, ng, acc):
            L.check(lib.csn_block_attn_bwd_dkv_f32(dd.data_ptr(), mstride, qd.data_ptr(), mstride, qi.data_ptr(), ld,
                                                   scb.ptr if scb else None, ds.ptr, dk.ptr, dv.ptr if dv else None, mstride,
                                                   ki.data_ptr(), ki.data_ptr() if dv else None, acc, ids.data_ptr(), n, H, d, T, nb,
                                                   Tp, 0, 0, 0, 0, 1, off.data_ptr() if off is not None else None, ng, _stream()),
                    "dkv")
        if grouped_dkv:
            call(kv_ids, E, kv_off, kv_ng, 0)
        else:
            for c, ev in enumerate(_colours(KV_IDX)):
                call(ev, ev.numel(), None, 0, int(c > 0))

    def dv_scores(scb, dv):
        L.check(lib.csn_block_attn_bwd_dv_scores_f32(dd.data_ptr(), mstride, ld, scb.ptr, lse.ptr, dv.ptr if hasattr(dv, "ptr") else
                                                     dv.data_ptr(), mstride, ki.data_ptr(), kv_ids.data_ptr(), E, H, d, T, nb, Tp, p,
                                                     seed, kv_off.data_ptr(), kv_ng, _stream()), "dv from scores")

    # ---- the current flow: P planes over the scores, two plane products
    scb1, ds1, delta1, dq1 = dq_call(1)
    dk1, dv1 = Canary(n_slots * mstride), Canary(n_slots * mstride)
    dkv_call(scb1, ds1, dk1, dv1)

    # ---- the three-call flow
    scb2, ds2, delta2, dq2 = dq_call(2)
    assert torch.equal(scb2.buf, sc.buf), "the dQ call without P planes touched the scores"
    assert torch.equal(dq2.buf, dq1.buf), "dQ differs"
    assert torch.equal(delta2.buf, delta1.buf), "delta differs"
    assert torch.equal(ds2.buf, ds1.buf), "the dS planes differ"
    dv2 = Canary(n_slots * mstride)
    dv_scores(scb2, dv2)
    dk2 = Canary(n_slots * mstride)
    dkv_call(None, ds2, dk2, None)
    assert torch.equal(dk2.buf, dk1.buf), "dK of the dK-only call differs from the two-product call"

    # ---- dV: what is written, against float64, against the plane route, repeatable
    used = sorted(set(KV_IDX))
    written = torch.zeros((n_slots, mstride), dtype=torch.bool, device="cuda")
    for s in used:
        written[s, :D * ld].view(D, ld)[:, :N] = True
    dv2.check(written, "dv from scores")
    keep, _ = ar.row_masks(r)
    ref = ar.block_attention_ref(*(ar.per_eval(t, ix, H).cuda() for t, ix in ((q, Q_IDX), (k, KV_IDX), (v, KV_IDX))),
                                 dctx.double().view(E, H, d, ld).cuda(), T, nb, Tl, keep, p)
    want = torch.zeros((n_slots, H, d, ld), dtype=torch.float64, device="cuda").index_add_(
        0, torch.tensor(KV_IDX, device="cuda"), ref["dv"])[used]
    maps = lambda c: c.f32().view(n_slots, -1)[:, :D * ld].view(n_slots, H, d, ld)[used]
    e_new = ar.per_block_err(maps(dv2), want, T, nb, Tl)
    e_old = ar.per_block_err(maps(dv1), want, T, nb, Tl)
    print(f"[dv-scores] {_case_id(r)}: dV error from scores {e_new:.3e}, plane route {e_old:.3e}")
    assert e_new <= 2.0 * e_old, f"dV from scores {e_new:.3e} > 2 x plane route {e_old:.3e}"
    assert e_new < ar.BOUNDS[1][1], f"dV from scores {e_new:.3e} >= {ar.BOUNDS[1][1]:.1e}"
    dv3 = Canary(n_slots * mstride)
    dv_scores(scb2, dv3)
    assert torch.equal(dv3.buf, dv2.buf), "dV from scores not repeatable"

    # ---- padding: a map whose rows run 8 points past the last one keeps exact zeros there (same pitch for dctx: a second set
    # of maps would cost a second forward, so only the OUTPUT pitch is what this checks — through the slot stride's tail)
    zbuf = torch.zeros((n_slots, mstride), device="cuda")
    dv_scores(scb2, zbuf)
    torch.cuda.synchronize()
    assert bool((zbuf[:, D * ld:] == 0).all()), "dV wrote past the maps"
    assert torch.equal(zbuf[used][:, :D * ld].view(torch.int32), dv2.f32().view(n_slots, -1)[used][:, :D * ld].view(torch.int32))


@pytest.mark.parametrize("pad", [8])
def test_dv_padding_columns_stay_zero(L, pad):
    """ld past n_blocks * block (points no block owns) and a short last block: the columns of dV beyond a block's T stay exact
    zeros in a zero-filled map, and the values equal those of the plane route's geometry (same error bound)."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    T, nb, d, H, E, S, p, seed = 132, 2, D_HEAD, 1, 4, 3, 0.1, 4242
    r = dict(mode=1, kv="tp", d=d, H=H, T=T, nb=nb, T_last=None, p=p, Tp=160, pad=pad, seed=seed, S=S, E=E, q_idx=Q_IDX, kv_idx=KV_IDX)
    N = nb * T
    ld, D, Tp = N + pad, d, 160
    q, k, v, dctx = ar.row_inputs(r)
    qi = torch.tensor(Q_IDX, dtype=torch.int32, device="cuda")
    ki = torch.tensor(KV_IDX, dtype=torch.int32, device="cuda")
    qd, dd = q.cuda().contiguous(), dctx.cuda().contiguous()
    ldp = nb * ar.BLOCK_PITCH * 2
    kv = ar.pack_tile_planes(torch.cat((k, v), 1), T, nb, 2, "bf16", None).cuda().contiguous()
    k_ptr, v_ptr = kv.data_ptr(), kv.data_ptr() + 2 * D * ldp
    ctx = torch.zeros((E, D, ld), device="cuda")
    lse = torch.zeros((E, H, nb * T), device="cuda")
    sc = torch.zeros((E, H, nb, T, Tp), device="cuda")
    L.check(lib.csn_block_attn_fwd_f32(qd.data_ptr(), k_ptr, v_ptr, D * ld, 2 * D * ldp, qi.data_ptr(), ki.data_ptr(), ld, ctx.data_ptr(),
                                       D * ld, sc.data_ptr(), lse.data_ptr(), E, H, d, T, nb, Tp, 8.0, p, seed, 1, ldp, _stream()), "forward")
    ids, off, ng = _groups(KV_IDX, S)
    dv = torch.zeros((S, D, ld), device="cuda")
    L.check(lib.csn_block_attn_bwd_dv_scores_f32(dd.data_ptr(), D * ld, ld, sc.data_ptr(), lse.data_ptr(), dv.data_ptr(), D * ld,
                                                 ki.data_ptr(), ids.data_ptr(), E, H, d, T, nb, Tp, p, seed, off.data_ptr(), ng,
                                                 _stream()), "dv from scores")
    torch.cuda.synchronize()
    assert bool((dv[..., N:] == 0).all()), "padding columns of dV are not exact zeros"
    keep, _ = ar.row_masks(r)
    ref = ar.block_attention_ref(*(ar.per_eval(t, ix, H).cuda() for t, ix in ((q, Q_IDX), (k, KV_IDX), (v, KV_IDX))),
                                 dctx.double().view(E, H, d, ld).cuda(), T, nb, None, keep, p)
    want = torch.zeros((S, H, d, ld), dtype=torch.float64, device="cuda").index_add_(0, torch.tensor(KV_IDX, device="cuda"), ref["dv"])
    e = ar.per_block_err(dv.view(S, H, d, ld), want, T, nb, None)
    print(f"[dv-scores] padded maps: dV error {e:.3e}")
    assert e < ar.BOUNDS[1][1]


def test_calls_are_refused_where_there_is_no_instance(L):
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    assert lib.csn_attn_bwd_dv_scores_available(256, 500) and not lib.csn_attn_bwd_dv_scores_available(128, 500)
    assert not lib.csn_attn_bwd_dv_scores_available(256, 516) and not lib.csn_attn_bwd_dv_scores_available(256, 502)
    z = torch.zeros(64, device="cuda")
    zp = z.data_ptr()
    assert lib.csn_block_attn_bwd_dv_scores_f32(zp, 0, 36, zp, zp, zp, 0, None, None, 1, 1, 128, 36, 1, 64, 0.0, 0, None, 0, _stream()) == -1
    L.check(lib.csn_set_math_mode(2))
    assert not lib.csn_attn_bwd_dv_scores_available(256, 500)
    assert lib.csn_block_attn_bwd_dv_scores_f32(zp, 0, 36, zp, zp, zp, 0, None, None, 1, 1, 256, 36, 1, 64, 0.0, 0, None, 0, _stream()) == -1


def test_module_step_with_dv_from_scores(L):
    """CrossShapeAt train-mode step, dv_from_scores on against off: the forward is untouched (logits and loss bit-equal); every
    gradient within the tolerance tests/test_gpu_flash.py::test_module_flows_agree uses between flows in math mode 1."""
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    from oracle import csa_oracle as orc
    L.check(L.lib().csn_set_math_mode(1))
    rng = np.random.default_rng(77)
    B, K, n_cls, C, N = 2, 1, 7, 256, 1000
    torch.manual_seed(5)
    model = get_model("csa", n_cls, 1, K, block=500, n_blocks=2).cuda().train(True)
    off = torch.from_numpy(rng.standard_normal((B, K + 1, C, 1, 1)).astype(np.float32))
    nbf = torch.from_numpy(rng.standard_normal((B, K + 1, C, N, 1)).astype(np.float32)) + 2.0 * off
    x = nbf[:, 0].contiguous()
    lab = torch.from_numpy(rng.integers(0, n_cls, size=(B, N)))
    outs = {}
    calls = []
    from csn_amd import _lib
    for on in (False, True):
        for prm in model.parameters():
            prm.grad = None
        torch.manual_seed(9)
        _lib.set_call_hook((lambda name, phase: calls.append(name) if phase == "begin" else None) if on else None)
        try:
            with tuning.override(dv_from_scores=on):
                logits = model(x.cuda(), "train", nbf.cuda())
                loss = orc.masked_ce_loss(logits, lab.cuda())
                loss.backward()
        finally:
            _lib.set_call_hook(None)
        outs[on] = (logits.detach(), loss.item(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert "csn_block_attn_bwd_dv_scores_f32" in calls, "the step did not take the dV-from-scores path"
    l0, s0, g0 = outs[False]
    l1, s1, g1 = outs[True]
    assert len(g0) == 11
    assert torch.equal(l0, l1) and s0 == s1
    for n in g0:
        scale = g0[n].abs().max().item()
        assert (g0[n] - g1[n]).abs().max().item() <= 5e-5 * scale, n
