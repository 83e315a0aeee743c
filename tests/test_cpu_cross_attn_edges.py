"""The host side of the cross-length / ragged attention sweep (tests/cross_attn_ref.py), checked without a GPU: the rectangular
reference against the block reference and plain torch, the launch's mask rule, the coverage of the two row tables, and the
sharpness of the probes — negative controls computed from the reference alone."""
import numpy as np
import pytest
import torch

from tests import attn_edge_ref as ar
from tests import cross_attn_ref as cr
from tests import dropout_ref as dr

CROSS, VARLEN = cr.cross_rows(), cr.varlen_rows()


def _f64(r, which=0):
    q, k, v, dctx = cr.cross_inputs(r, which)
    E, H, d = r["E"], r["H"], r["d"]
    return tuple(t.double().view(E, H, d, -1) for t in (q, k, v, dctx))


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,p", [(36, 0.0), (64, 0.3), (100, 0.1)])
def test_rectangular_reference_equals_the_block_reference_on_square_cases(T, p):
    r = dict(kind="cross", mode=0, d=32, H=2, E=2, nq=[T] * 2, nk=[T] * 2, Tp=ar.ceil_to(T, 32), ld_q=T, ld_kv=T, seed=77, p=p)
    q, k, v, dctx = _f64(r)
    keep = cr.row_keep(r)
    got = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep, p)
    bk = ar.block_keep(2, 2, T, 1, r["Tp"], 77, p)
    want = ar.block_attention_ref(q, k, v, dctx, T, 1, None, bk, p)
    if keep is not None:
        assert torch.equal(keep, bk[:, :, 0])
    for e in range(2):
        for n in ("ctx", "dq", "dk", "dv", "lse"):
            assert torch.equal(got[e][n], want[n][e]), n
        for n in ("S", "P", "dS"):
            assert torch.equal(got[e][n], want[n][e, :, 0]), n


def test_rectangular_reference_equals_plain_torch_attention():
    r = dict(kind="cross", mode=0, d=64, H=2, E=3, nq=[8, 132, 4], nk=[37, 5, 1], Tp=40, ld_q=140, ld_kv=52, seed=5, p=0.3)
    q, k, v, dctx = _f64(r)
    keep = cr.row_keep(r)
    ref = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep, r["p"])
    for e, (n, m) in enumerate(zip(r["nq"], r["nk"])):
        qe, ke, ve, de = q[e, :, :, :n], k[e, :, :, :m], v[e, :, :, :m], dctx[e, :, :, :n]
        s = qe.transpose(-1, -2) @ ke
        pr = torch.softmax(s, -1)
        md = keep[e, :, :n, :m].double() / (1 - r["p"])
        ctx = ve @ (pr * md).transpose(-1, -2)
        dp = de.transpose(-1, -2) @ ve
        delta = (de * ctx).sum(-2)
        ds = pr * (dp * md - delta.unsqueeze(-1))
        assert ref[e]["ctx"].shape == (2, 64, n) and ref[e]["dk"].shape == (2, 64, m)
        for name, want in (("ctx", ctx), ("S", s), ("P", pr * md), ("lse", torch.logsumexp(s, -1)), ("delta", delta), ("dS", ds),
                           ("dq", ke @ ds.transpose(-1, -2)), ("dk", qe @ ds), ("dv", de @ (pr * md))):
            assert torch.allclose(ref[e][name], want, atol=1e-10, rtol=0), name
    # a one-key evaluation: dS, dQ, dK are exactly zero
    assert all(float(ref[2][n].abs().max()) == 0.0 for n in ("dS", "dq", "dk"))
    # float32 evaluation of the same formula (the err32 yardstick) is the same thing to fp32 rounding, and results do not
    # depend on the sentinels
    r32 = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep, r["p"], dtype=torch.float32)
    assert 0 < cr.eval_err(r32[0]["ctx"], ref[0]["ctx"]) < 1e-5
    other = cr.cross_attention_ref(*_f64(r, 1), r["nq"], r["nk"], keep, r["p"])
    assert all(torch.equal(other[e][n], ref[e][n]) for e in range(3) for n in ref[e])


def test_launch_mask_is_the_transposed_attention_mask_with_the_launch_pitch():
    E, H, seed, p = 2, 2, cr.HIGH_SEED, 0.3
    m = cr.launch_keep(E, H, 132, 37, 64, seed, p)
    want = dr.attention_mask(E, H, 1, 37, 64, seed, p, Tq=132)[:, :, 0]
    assert m.shape == (E, H, 132, 37) and np.array_equal(m.numpy(), want.transpose(0, 1, 3, 2))
    assert torch.equal(cr.launch_keep(E, H, 132, 37, 64, seed, p, shift=1)[..., :-1], m[..., 1:])
    # more queries than the pitch: the mask of pitch n_queries, which is not the one drawn with pitch score_pitch
    big = cr.launch_keep(E, H, 1000, 37, 40, seed, p)
    wrong = cr.launch_keep(E, H, 1000, 37, 40, seed, p, mask_pitch=40)           # the pitch a kernel would take from score_pitch
    assert np.array_equal(big.numpy(), dr.attention_mask(E, H, 1, 37, 1000, seed, p, Tq=1000)[:, :, 0].transpose(0, 1, 3, 2))
    assert np.array_equal(wrong.numpy()[:, :, :40], dr.attention_mask(E, H, 1, 37, 40, seed, p, Tq=40)[:, :, 0].transpose(0, 1, 3, 2))
    differ = (big != wrong)[..., 2:].double().mean().item()                      # (the key pair 0 has pair index = query on any pitch)
    assert 0.3 < differ < 0.5                                                    # 2 p (1 - p) = 0.42 of the positions
    p1 = 0.1
    d1 = (cr.launch_keep(E, H, 1000, 37, 40, seed, p1) != cr.launch_keep(E, H, 1000, 37, 40, seed, p1, mask_pitch=40))
    assert 0.14 < d1.double().mean().item() < 0.20                               # 17 % at the layer's dropout rate


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def test_row_tables_cover_every_class():
    assert 150 <= len(CROSS) <= 200 and 20 <= len(VARLEN) <= 30
    classes = {cr.key_class(nk) for nk in cr.KEY_COUNTS}
    assert classes == set(cr.KEY_CLASSES)
    assert any(nk % 4 for nk in cr.KEY_COUNTS if nk > 512) and {nk % 32 for nk in cr.KEY_COUNTS} >= {0, 1, 31}
    for rows in (CROSS, VARLEN):
        for mode in (0, 1):
            for d in cr.DIMS:
                sel = [r for r in rows if (r["mode"], r["d"]) == (mode, d)]
                if rows is CROSS:
                    assert {r["nk"][0] for r in sel} == set(cr.KEY_COUNTS), (mode, d)
                    assert {cr.key_class(r["nk"][0]) for r in sel} == classes
                    assert {r["pitch"] for r in sel} == set(cr.PITCHES), (mode, d)
                    assert any(r["nq"][0] > r["nk"][0] for r in sel) and any(r["nq"][0] < r["nk"][0] for r in sel)
                    assert {0.0, 0.1} <= {r["p"] for r in sel}
                else:
                    assert {r["pitch"] for r in sel} == set(cr.VARLEN_PITCHES), (mode, d)
                # both data flows of the backward wherever the mode has two
                flows = {cr.planes_flow(mode, r["Tp"], max(r["nk"])) for r in sel}
                assert flows == ({False} if mode == 0 else {False, True}), (mode, d)
    assert {r["nq"][0] for r in CROSS} == set(cr.QUERY_COUNTS) | {cr.MANY_QUERIES}
    for mode in (0, 1):                                                     # 1000 queries on a pitch below them, at live dropout
        assert any(r["mode"] == mode and r["nq"][0] > r["Tp"] and r["p"] > 0 for r in CROSS)
        assert any(r["mode"] == mode and r["nq"][0] == 1000 and r["nk"][0] == 1301 for r in CROSS)
    for rows in (CROSS, VARLEN):
        assert {r["H"] for r in rows} == {1, 2, 8} and all(r["H"] != 8 or r["d"] == 32 for r in rows)
        assert {r["p"] for r in rows} == {0.0, 0.1, 0.5}
        assert any(r["seed"] >> 32 for r in rows) and any(not r["seed"] >> 32 for r in rows)
        assert any(r["ld_q"] > max(r["nq"]) for r in rows) and any(r["ld_q"] == max(r["nq"]) for r in rows)
        assert any(r["ld_kv"] > ar.ceil_to(max(r["nk"]), 4) for r in rows) and any(r["ld_kv"] == ar.ceil_to(max(r["nk"]), 4) for r in rows)
        assert any(r["q_stride"] > r["H"] * r["d"] * r["ld_q"] for r in rows)
        assert any(r["kv_stride"] > r["H"] * r["d"] * r["ld_kv"] for r in rows)
        for r in rows:
            assert r["Tp"] % 4 == 0 and r["Tp"] >= ar.ceil_to(max(r["nk"]), 4) and all(n % 4 == 0 for n in r["nq"])
    assert {r["E"] for r in CROSS} == {2, 3}
    assert CROSS[-1]["nk"][0] == max(cr.KEY_COUNTS) and max(VARLEN[-1]["nk"]) == max(cr.KEY_COUNTS)      # the largest rows last
    for r in VARLEN:
        assert 5 <= r["E"] <= 6
        assert len(set(r["nq"])) == r["E"] and len(set(r["nk"])) == r["E"]              # all counts of a batch differ
        assert 1 in r["nk"] and 4 in r["nq"] and max(r["nq"]) > 256
        assert r["nk"][0] != max(r["nk"]) and r["nq"][0] != max(r["nq"])                 # the longest not first
        assert len({cr.key_class(n) for n in r["nk"]}) >= 3 and any(n % 4 for n in r["nk"])
    assert {cr.key_class(n) for r in VARLEN for n in r["nk"]} == classes
    assert any(max(r["nq"]) > r["Tp"] and r["p"] > 0 and r["mode"] == m for r in VARLEN for m in (0, 1))
    other = cr.other_mode_rows()
    assert 8 <= len(other) <= 12 and all(r["mode"] == 1 for r in other)
    assert {r["kind"] for r in other} == {"cross", "varlen"} and any(r["p"] > 0 for r in other)
    assert {cr.planes_flow(1, r["Tp"], max(r["nk"])) for r in other} == {False, True}
    again = cr.resentinel_rows()
    assert all(r["ld_kv"] > min(r["nk"]) for r in again) and any(r["ld_q"] > min(r["nq"]) for r in again)
    assert {r["nk"][0] % 4 != 0 for r in again if r["kind"] == "cross"} == {False, True}
    assert 6 <= len(again) <= 16 and {r["kind"] for r in again} == {"cross", "varlen"} and {r["mode"] for r in again} == {0, 1}


def test_written_regions():
    r = dict(E=2, H=2, d=32, nq=[8, 4], nk=[37, 1], Tp=64, ld_q=12, ld_kv=44, q_stride=2 * 32 * 12 + 16, kv_stride=2 * 32 * 44)
    w = cr.map_written(r, keys=False).view(2, -1)
    assert int(w[0].sum()) == 64 * 8 and int(w[1].sum()) == 64 * 4 and not w[:, 64 * 12:].any()
    assert w[0, :64 * 12].view(64, 12)[:, :8].all() and not w[0, :64 * 12].view(64, 12)[:, 8:].any()
    wk = cr.map_written(r, keys=True)
    assert int(wk[0].sum()) == 64 * 40 and int(wk[1].sum()) == 64 * 4
    assert int(cr.stat_written(r).sum()) == 2 * (8 + 4)
    assert int(cr.score_written(r, False).sum()) == 2 * (8 * 40 + 4 * 4) and int(cr.score_must(r).sum()) == 2 * (8 * 37 + 4 * 1)
    assert int(cr.score_written(r, True).sum()) == 2 * (8 * 64 + 4 * 32)


# ---- negative controls ------------------------------------------------------------------------------------------------------------
def _gaps(ref, ctl, rows_sel):
    """smallest difference of the control from the reference over the selected (head, query) rows of one evaluation, relative
    to the head's max |ctx|; rows_sel (H, nq) bool.  None when no row is selected."""
    n = min(ref.shape[-1], ctl.shape[-1])
    scale = ref.abs().amax((-1, -2))
    diff = (ctl[..., :n] - ref[..., :n]).abs().amax(-2) / scale[:, None]                # (H, n)
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    sel = rows_sel[:, :n]
    return diff[sel].min().item() if sel.any() else None


def _mask_rows(r, e, keep, other):
    """the spike rows of evaluation e whose spiked key's keep decision the two masks decide differently"""
    nq, nk = r["nq"][e], r["nk"][e]
    roles = torch.from_numpy(ar.query_roles(nq))
    kl, kf = ar.probe_keys(nk)
    sel = torch.zeros((r["H"], nq), dtype=torch.bool)
    for role, key in ((ar.ROLE_LAST, kl), (ar.ROLE_TILE, kf), (ar.ROLE_FIRST, 0)):
        rows = torch.nonzero(roles == role)[:, 0]
        sel[:, rows] |= keep[e][:, rows, key] != other[e][:, rows, key]
    return sel


def _controls(r):
    """{control: smallest gap over the evaluations and probe rows where it applies (None: nowhere)}"""
    q, k, v, dctx = _f64(r)
    nq, nk, p, H = r["nq"], r["nk"], r["p"], r["H"]
    keep = cr.row_keep(r)
    fwd = lambda **kw: [o["ctx"] for o in cr.cross_attention_ref(q, k, v, dctx, kw.pop("nq", nq), kw.pop("nk", nk),
                                                                 kw.pop("keep", keep), p, grads=False, **kw)]
    ref = fwd()
    gaps = {}

    def note(name, g):
        if g is not None:
            gaps[name] = min(gaps.get(name, float("inf")), g)

    last, pad = fwd(drop_last_key=True), fwd(pad_key=cr.key_sentinel(H, r["d"]))
    wide = max(nq) > r["Tp"]
    if keep is not None:
        # the mask with the wrong pitch where the query count exceeds score_pitch, shifted by one key elsewhere
        other = cr.row_keep(r, mask_pitch=r["Tp"]) if wide else cr.row_keep(r, shift=1)
        masked = fwd(keep=other)
    for e in range(r["E"]):
        roles = torch.from_numpy(ar.query_roles(nq[e]))
        kl, _ = ar.probe_keys(nk[e])
        live = keep[e][:, :nq[e], :nk[e]].any(-1) if keep is not None else torch.ones((H, nq[e]), dtype=torch.bool)
        kept = keep[e][:, :nq[e], kl] if keep is not None else live
        note("last key", _gaps(ref[e], last[e], (roles == ar.ROLE_LAST)[None] & kept))
        # (the padding key is kept by the mask: it takes over a ROLE_NEG row whether or not the row keeps a real key)
        note("padding", _gaps(ref[e], pad[e], (roles == ar.ROLE_NEG)[None].expand(H, -1)))
        if keep is not None:
            note("wrong pitch" if wide else "shift", _gaps(ref[e], masked[e], _mask_rows(r, e, keep, other)))
    if r["kind"] == "varlen":
        E = r["E"]
        nb_q, nb_k = [nq[(e + 1) % E] for e in range(E)], [nk[(e + 1) % E] for e in range(E)]
        # an evaluation computed with its neighbour's counts: the neighbour's keys (fewer: real keys lost; more: padding keys
        # let in) on the rows both have — the rows it has not are missing or written outside the region, which the canaries see
        neigh = fwd(nq=[min(a, b) for a, b in zip(nq, nb_q)], nk=nb_k)
        for e in range(E):
            roles = torch.from_numpy(ar.query_roles(nq[e]))
            if nb_k[e] < nk[e] and keep is not None:                          # (a lost key only shows where the mask kept it)
                probe = (roles == ar.ROLE_LAST)[None] & keep[e][:, :nq[e], nk[e] - 1]
            elif nb_k[e] < nk[e]:
                probe = (roles == ar.ROLE_LAST)[None].expand(H, -1)
            else:
                probe = (roles == ar.ROLE_NEG)[None].expand(H, -1)
            note("neighbour's counts", _gaps(ref[e], neigh[e], probe))
        if keep is not None and wide:
            # the mask drawn with the evaluation's own query count instead of max_queries
            own = [cr.launch_keep(E, H, max(nq), max(nk), r["Tp"], r["seed"], p, mask_pitch=max(nq[e], r["Tp"]))[e] for e in range(E)]
            own_ctx = fwd(keep=torch.stack(own))
            for e in range(E):
                if max(nq[e], r["Tp"]) != max(nq):
                    note("own query count", _gaps(ref[e], own_ctx[e], _mask_rows(r, e, keep, torch.stack(own))))
    return gaps


def _control_rows():
    """every (3c) launch; of (3b) every key count, pitch class, dropout rate and the 1000-query rows at head widths 32 and 256
    (the probes depend on the width only through their noise) — without the 1000 x 1301 rows' siblings at other widths"""
    return [r for r in CROSS if r["d"] in (32, 256)] + VARLEN


def test_negative_controls_are_sharp():
    """A reference that lost the last valid key, let the padding key (the sentinel of column nk) in, drew the keep mask with
    the wrong pitch or shifted by one key, computed an evaluation of a ragged batch with its neighbour's counts or drew its
    mask with its own query count lies >= 10x the mode's forward bound from the true reference on every probe row where the
    control applies (relative to the head's max |ctx|)."""
    seen = {}
    applied = {"shift": 0, "wrong pitch": 0}
    n_drop = 0
    for r in _control_rows():
        need = 10 * ar.BOUNDS[r["mode"]][0]
        gaps = _controls(r)
        assert {"last key", "padding"} <= set(gaps), cr.row_id(r)
        if r["kind"] == "varlen":
            assert "neighbour's counts" in gaps, cr.row_id(r)
            if r["p"] > 0 and max(r["nq"]) > r["Tp"]:
                assert {"wrong pitch", "own query count"} <= set(gaps), cr.row_id(r)
        if r["p"] > 0:
            n_drop += 1
            # (keys 0 and 1 have pair index = query on any pitch: the pitch shows from key 2 on)
            if max(r["nq"]) > r["Tp"] and max(r["nq"]) >= 128 and max(r["nk"]) > 2:
                assert "wrong pitch" in gaps, cr.row_id(r)
        for name, g in gaps.items():
            assert g >= need, (cr.row_id(r), name, g, need)
            seen[name] = min(seen.get(name, float("inf")), g)
            if name in applied:
                applied[name] += 1
    assert set(seen) == {"last key", "padding", "shift", "wrong pitch", "neighbour's counts", "own query count"}
    # a mask control needs a spike row whose spiked key the two masks decide differently: a 4-query row at p = 0.1 may have
    # none.  Most dropout rows have one
    assert applied["shift"] + applied["wrong pitch"] >= 0.7 * n_drop, (applied, n_drop)
    print("[cross-edge controls] smallest gaps:", {n: f"{g:.2e}" for n, g in seen.items()})


def _row_condition(r):
    q, k, v, dctx = _f64(r)
    keep = cr.row_keep(r)
    ref = cr.cross_attention_ref(q, k, v, dctx, r["nq"], r["nk"], keep, r["p"])
    return cr.row_condition(r, ref, q, k, v, dctx, keep)


def test_every_draw_is_well_conditioned():
    """Every row's inputs, at the draw the table lists for it, keep every gradient of every (evaluation, head) within
    COND_LIMIT of the size of its terms (cross_attn_ref.condition: from the float64 reference alone), so that an error relative
    to max |reference| measures the kernel; and REDRAW lists only rows whose earlier draws are beyond the limit — among them
    a 4 x 2 evaluation whose single gradient row has dS 170x smaller than its terms."""
    worst = 0.0
    for r in CROSS + VARLEN:
        c = _row_condition(r)
        assert max(c.values()) <= cr.COND_LIMIT, (cr.row_id(r), c)
        worst = max(worst, max(c.values()))
        assert r["redraw"] == cr.REDRAW.get(r["i"], 0)
        for draw in range(r["redraw"]):
            assert max(_row_condition(dict(r, redraw=draw)).values()) > cr.COND_LIMIT, (cr.row_id(r), draw)
    assert set(cr.REDRAW) <= {r["i"] for r in CROSS + VARLEN} and len(cr.REDRAW) <= 4
    assert max(_row_condition(dict(CROSS[15], redraw=0)).values()) > 100
    print(f"[cross-edge conditioning] worst accepted {worst:.2f}")


def test_removing_a_key_count_class_fails_the_coverage():
    """the coverage test is an assertion about the table, not a restatement of it: without the 37-key rows it fails"""
    full = list(CROSS)
    try:
        CROSS[:] = [r for r in full if r["nk"][0] != 37]
        with pytest.raises(AssertionError):
            test_row_tables_cover_every_class()
    finally:
        CROSS[:] = full
