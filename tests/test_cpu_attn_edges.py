"""The host side of the attention edge sweep (tests/attn_edge_ref.py), checked without a GPU: the tile-plane packer against the
contract, the short-block mask rule, the sharpness of the probes (negative controls) and the coverage of the row table."""
import numpy as np
import pytest
import torch

from tests import attn_edge_ref as ar
from tests import dropout_ref as dr


@pytest.mark.parametrize("npl,fmt,tol", [(2, "bf16", 2.0 ** -16), (1, "bf16", 2.0 ** -8), (1, "f16", 2.0 ** -11)])
@pytest.mark.parametrize("T,nb,T_last", [(36, 3, None), (64, 2, None), (500, 2, 100), (28, 2, 4), (4, 3, None)])
def test_tile_plane_packer(npl, fmt, tol, T, nb, T_last):
    rng = np.random.default_rng(T + nb)
    N = ar.n_points(T, nb, T_last)
    x = torch.from_numpy(rng.standard_normal((2, 3, N + 8)).astype(np.float32))
    planes = ar.pack_tile_planes(x, T, nb, npl, fmt, T_last)
    assert planes.dtype == torch.int16 and planes.shape == (2, 3, nb * 512 * npl)
    vals = ar.unpack_tile_planes(planes, nb, npl, fmt)
    for b, Tb in enumerate(ar.block_lengths(T, nb, T_last)):
        src = x[..., b * T: b * T + Tb]
        got = vals[:, :, b, :Tb]
        assert ((got - src).abs() <= tol * src.abs()).all()
        end = ar.ceil_to(Tb, ar.KT)
        assert (vals[:, :, b, Tb:end] == 0).all()                           # padding keys of the last tile: zeros
        assert torch.isnan(vals[:, :, b, end:]).all()                        # tiles past the last: NaN (never read)
        raw = planes.view(2, 3, nb, 16, npl, ar.KT)[:, :, b, end // ar.KT:]
        assert (raw == (ar.NAN_BF16 if fmt == "bf16" else ar.NAN_F16)).all()
    if npl == 2:                                                            # [hi 32 | lo 32]: hi = bf16(x), lo = bf16(x - hi)
        hi = planes.view(2, 3, nb, 16, 2, ar.KT)[:, :, 0, 0, 0].view(torch.bfloat16)
        n0 = min(ar.block_lengths(T, nb, T_last)[0], ar.KT)
        assert torch.equal(hi[..., :n0], x[..., :n0].bfloat16())


@pytest.mark.parametrize("T,Tp,T_last", [(36, 64, 4), (60, 64, 28), (508, 512, 100), (260, 320, 36)])
def test_short_block_mask_rule(T, Tp, T_last):
    """The mask of a short last block is the full block's mask cut to T_last keys and queries: the pair index is
    key / 2 * max(score_pitch, block) + query whatever the block holds (attn_f32.hip, attn_bf16x3.hip, attn_dkv.hip all take the
    pitch from the full block).  attention_mask drawn for the short block with the full block's query count agrees; drawn with
    the short block's own query count (pitch max(Tp, T_last) = Tp here) it agrees too because Tp >= T — the rule only matters
    for the pitch, which the score buffer fixes."""
    E, H, nb, seed, p = 2, 2, 3, 0xdead_beef_0123_4567, 0.3
    full = ar.block_keep(E, H, T, nb, Tp, seed, p)                          # [e][h][blk][query][key]
    cut = dr.attention_mask(E, H, nb, T_last, Tp, seed, p, Tq=T)[..., :T_last]          # [key][query]
    assert np.array_equal(full[:, :, -1, :T_last, :T_last].numpy(), cut[:, :, -1].transpose(0, 1, 3, 2))
    ext = ar.block_keep(E, H, T, nb, Tp, seed, p, extra_keys=1)
    assert torch.equal(ext[..., :T], full)
    assert 0.6 < full.double().mean().item() < 0.8


def _controls(r):
    q, k, v, dctx = ar.row_inputs(r)
    H, d, ld = r["H"], r["d"], q.shape[-1]
    keep, shifted = ar.row_masks(r)
    return ar.control_gaps(ar.per_eval(q, r["q_idx"], H), ar.per_eval(k, r["kv_idx"], H), ar.per_eval(v, r["kv_idx"], H),
                           dctx.double().view(r["E"], H, d, ld), r["T"], r["nb"], r["T_last"], keep, shifted, r["p"])


def test_negative_controls_are_sharp():
    """On the probe rows of the sweep's rows (every block length, short last block, dropout rate and score pitch; head widths
    32 and 256 — the probes depend on the width only through their noise — and every width of the widest bound, mode 2), a
    reference that lost the last valid key, that let one padding key in, or whose mask is shifted by one key differs from the
    true reference by >= 10x the mode's forward bound (relative to the block's max): a kernel with any of these errors fails
    the sweep, without a kernel having to be broken to show it."""
    worst = {}
    for r in ar.rows():
        if r["d"] not in (32, 256) and r["mode"] != 2:     # the probes do not depend on the head width beyond its noise
            continue
        need = 10 * ar.BOUNDS[r["mode"]][0]
        gaps = _controls(r)
        for name, g in gaps.items():
            if name == "shift" and r["p"] == 0:
                assert g is None
                continue
            assert g is not None, (ar.row_id(r), name)
            assert g >= need, (ar.row_id(r), name, g, need)
            worst[name] = min(worst.get(name, 1e9), g)
    assert set(worst) == {"last key", "padding", "shift"}


def test_probe_rows_and_dropped_probe_keys():
    """The last query row of every block is a probe row, every block has rows of every role, and in every dropout row some
    probe keys are dropped and some kept."""
    for Tb in (4, 28, 32, 36, 100, 500):
        roles = ar.query_roles(Tb)
        assert roles[-1] == ar.ROLE_LAST and roles[-2] == ar.ROLE_NEG
        assert {ar.ROLE_LAST, ar.ROLE_TILE, ar.ROLE_NEG} <= set(roles.tolist())
    for r in ar.rows():
        keep, _ = ar.row_masks(r)
        if keep is None:
            continue
        kept = dropped = 0
        for b, Tb in enumerate(ar.block_lengths(r["T"], r["nb"], r["T_last"])):
            roles = ar.query_roles(Tb)
            kl, kf = ar.probe_keys(Tb)
            for role, key in ((ar.ROLE_LAST, kl), (ar.ROLE_TILE, kf)):
                rows = torch.from_numpy(np.nonzero(roles == role)[0])
                sel = keep[:, :, b, rows, key]
                kept += int(sel.sum())
                dropped += int((~sel).sum())
        assert kept > 0 and dropped > 0, ar.row_id(r)


def test_row_table_covers_every_instance_and_edge():
    """Computed from the table: every instance (math mode x K / V form) at every head width meets every block length, every
    short last block and dropout 0 / 0.1; dropout 0.5, a seed with its high 32 bits set, a score pitch past the round-up of
    the block, H = 8 at d = 32; and every call form csn_attn_bwd_grouping offers (restated as data) appears at every width
    where it exists."""
    rows = ar.rows()
    want_T = {T for T, _ in ar.BLOCKS}
    for mode, kv in ar.INSTANCES:
        for d in ar.DIMS:
            sel = [r for r in rows if (r["mode"], r["kv"], r["d"]) == (mode, kv, d)]
            assert {r["T"] for r in sel} == want_T, (mode, kv, d)
            assert {r["T_last"] for r in sel if r["T_last"]} == set(ar.SHORT_LAST)
            assert {0.0, 0.1} <= {r["p"] for r in sel}
            assert any(r["p"] > 0 and r["T_last"] for r in sel)
            offered = set()
            for r in sel:
                g = ar.grouping(mode, d, r["T"])
                offered |= {n for bit, n in ((2, "dkv_grouped"), (4, "dq_recompute"), (8, "flash"), (16, "tile_major")) if g & bit}
                assert ar.forms(r) >= ({"fwd", "fwd_noscores"} | ({"dq", "dkv"} if mode == 0 or kv == "f32" else set()))
            covered = set().union(*(ar.forms(r) for r in sel))
            if mode in (1, 2) and kv == "tp":
                assert offered <= covered and {"dq_tiles", "dq_grouped", "dkv_tiles"} <= covered
            if mode == 3:
                assert covered == {"fwd", "fwd_noscores"}
    assert any(r["p"] == 0.5 for r in rows)
    assert any(r["seed"] >> 32 for r in rows)
    assert any(r["Tp"] > ar.ceil_to(r["T"], ar.KT) for r in rows)
    assert any(r["d"] == 32 and r["H"] == 8 for r in rows)
    assert any(r["pad"] for r in rows)                                      # points past n_blocks * block (the ctx canary)
    # the forms of the headline instance: bf16x3, d = 256, tile planes — tile-major scores, grouped dK / dV
    assert any("tile_major" in ar.forms(r) and r["d"] == 256 and r["p"] > 0 and r["T_last"] for r in rows)
    # flash and recompute exactly where the library has them: mode 1 up to d = 128, mode 2 at every width (no flash at 256)
    assert ar.grouping(1, 256, 500) & 4 == 0 and ar.grouping(2, 256, 500) & 4 and not ar.grouping(2, 256, 500) & 8
    assert ar.grouping(1, 128, 36) & 8 and ar.grouping(0, 64, 100) == 0
    # the rescale branch: at d = 256 with tile planes the last (partial) tile of a multi-tile block holds a spiked key
    r = next(r for r in rows if (r["mode"], r["kv"], r["d"], r["T"]) == (1, "tp", 256, 260))
    kl, kf = ar.probe_keys(r["T"])
    assert kf == 256 and kl == 259 and ar.ROLE_FIRST in ar.query_roles(r["T"])


def test_reference_grads_are_autograd_of_the_explicit_formulas():
    """The reference's dS / dQ / dK / dV are those of the explicit softmax-backward formulas (with a short block and dropout)."""
    r = dict(ar.rows()[7], mode=0)
    q, k, v, dctx = ar.row_inputs(r)
    H, d, T, nb, Tl, p = r["H"], r["d"], r["T"], r["nb"], r["T_last"], 0.3
    keep = ar.block_keep(r["E"], H, T, nb, r["Tp"], r["seed"], p)
    qe, ke, ve = ar.per_eval(q, r["q_idx"], H), ar.per_eval(k, r["kv_idx"], H), ar.per_eval(v, r["kv_idx"], H)
    de = dctx.double().view(r["E"], H, d, -1)
    ref = ar.block_attention_ref(qe, ke, ve, de, T, nb, Tl, keep, p)
    for b, Tb in enumerate(ar.block_lengths(T, nb, Tl)):
        c = slice(b * T, b * T + Tb)
        s = qe[..., c].transpose(-1, -2) @ ke[..., c]
        pr = torch.softmax(s, -1)
        m = keep[:, :, b, :Tb, :Tb].double() / (1 - p)
        dp = de[..., c].transpose(-1, -2) @ ve[..., c]
        ds = pr * (dp * m - ((pr * m) * dp).sum(-1, keepdim=True))
        assert torch.allclose(ref["dS"][:, :, b, :Tb, :Tb], ds, atol=1e-10)
        assert torch.allclose(ref["dq"][..., c], ke[..., c] @ ds.transpose(-1, -2), atol=1e-10)
        assert torch.allclose(ref["dv"][..., c], de[..., c] @ (pr * m), atol=1e-10)
