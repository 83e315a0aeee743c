"""The host side of the 16-bit activation-map edge tests (tests/act16_ref.py), checked without a GPU: the flush of the fp16-forward
rows keeps every probe, the 16-bit written mask is the fp32 map's, and the derived bounds of the out-projection + LayerNorm cases
are both SHARP (a point, a channel row or the last 8-byte unit of a row dropped on float64 data costs at least 10x the bound, on
every shape) and SOUND for the arithmetic they describe (a float32 restatement stays under them)."""
import numpy as np
import pytest
import torch

from tests import act16_ref as a16
from tests import attn_edge_ref as ar

ROWS2 = [r for r in ar.rows() if r["mode"] == 2 and r["kv"] == "tp"]


def test_the_rows_are_the_issues_fifty():
    assert len(ROWS2) == 50
    assert {r["d"] for r in ROWS2} == set(ar.DIMS) and {(r["T"], r["T_last"]) for r in ROWS2} == set(ar.BLOCKS)
    assert any(r["p"] > 0 for r in ROWS2) and any(r["pad"] for r in ROWS2) and all(len(set(r["q_idx"])) < r["E"] for r in ROWS2)


@pytest.mark.parametrize("r", ROWS2[::7] + [ROWS2[-1]], ids=lambda r: ar.row_id(r))
def test_flush_keeps_the_probes(r):
    """|v| < 2^-14 -> 0 leaves every map exact in fp16 and in bf16 and changes no probe key, no spike and no role: the probe
    channels of q and k, the offset channels of v and the zero columns of dctx are the same bits before and after."""
    raw = ar.row_inputs(r)
    got = a16.flushed_row_inputs(r)
    S, H, d = r["S"], r["H"], r["d"]
    for x, y in zip(raw, got):
        assert torch.equal(ar.round16(y, "f16"), y) and torch.equal(ar.round16(y, "bf16"), y)
        changed = x != y
        assert bool((x[changed].abs() < a16.F16_MIN).all()) and bool((y[changed] == 0).all())
        assert changed.double().mean().item() < 1e-3                       # noise values only: a handful per map
    q, k, v, dctx = (t.view(t.shape[0], H, d, -1) for t in got)
    q0, k0, v0, d0 = (t.view(t.shape[0], H, d, -1) for t in raw)
    assert torch.equal(q[:, :, :4], q0[:, :, :4]) and torch.equal(k[:, :, :4], k0[:, :, :4])
    assert torch.equal(v[:, :, ar.OFF], v0[:, :, ar.OFF])
    assert bool((dctx[d0 == 0] == 0).all())                                # the spike rows and the offset channels stay the zeros
    for b, Tb in enumerate(ar.block_lengths(r["T"], r["nb"], r["T_last"])):
        c0 = b * r["T"]
        kl, kf = ar.probe_keys(Tb)
        roles = ar.query_roles(Tb)
        assert bool((k[:, :, ar.CH_LAST, c0 + kl] == 1).all()) and bool((k[:, :, ar.CH_TILE, c0 + kf] == 1).all())
        assert bool((k[:, :, ar.CH_NEG, c0:c0 + Tb] == ar.NEG_K).all())
        for role, ch, val in ((ar.ROLE_LAST, ar.CH_LAST, ar.SPIKE), (ar.ROLE_NEG, ar.CH_NEG, -ar.SPIKE / ar.NEG_K)):
            cols = c0 + np.nonzero(roles == role)[0]
            assert bool((q[:, :, ch, cols] == val).all())


def test_written_mask_of_a_16bit_map(monkeypatch):
    """map_written16 against the sweep's own _map_written, element for element: the first half of the buffer (in 16-bit elements)
    carries the fp32 map's mask, the second half nothing."""
    zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: zeros(*a, **{**k, "device": "cpu"}))
    from tests.test_gpu_attn_edges import _map_written
    for n_slots, slots, D, ld, N in ((3, range(3), 64, 40, 36), (3, [0, 1], 256, 528, 520), (4, [2], 32, 4, 4)):
        stride = D * ld + 16
        want = _map_written(n_slots, slots, stride, D, ld, N)
        got = a16.map_written16(n_slots, slots, stride, D, ld, N)
        assert got.shape == (2 * n_slots * stride,)
        assert torch.equal(got[:n_slots * stride].view(n_slots, stride), want) and not bool(got[n_slots * stride:].any())
        assert torch.equal(a16.map_written(n_slots, slots, stride, D, ld, N), want)


def test_16bit_canary_check_sees_one_element():
    body = torch.full((40,), ar.CANARY32, dtype=torch.int32)
    w = torch.zeros(80, dtype=torch.bool)
    w[:10] = True
    assert a16.touched16(body, w) == 0
    h = body.view(torch.int16)
    h[3] = 0x3F80                                     # inside the written region
    assert a16.touched16(body, w) == 0
    h[10] = 0x3F80                                    # the first element past it: what a write of fp32 width would reach
    h[79] = 0
    assert a16.touched16(body, w) == 2
    assert np.isnan(a16.widen16(torch.tensor([a16.nan16("bf16")], dtype=torch.int16), "bf16").item())
    assert np.isnan(a16.widen16(torch.tensor([a16.nan16("f16")], dtype=torch.int16), "f16").item())


# ---- the derived bounds of the out-projection + LayerNorm cases --------------------------------------------------------------
CASES = [(i, fmt) for i in range(len(a16.OUTPROJ_SHAPES)) for fmt in ("bf16", "f16")]


def _mutations(c):
    NP = c["NP"]
    return {"point": dict(n_keep=NP - 1), "row": dict(drop_row=True), "unit": dict(n_keep=NP - 4)}


@pytest.mark.parametrize("i,fmt", CASES, ids=[f"{a16.outproj_id(i)}-{f}" for i, f in CASES])
def test_outproj_bounds_are_sharp_and_sound(i, fmt):
    c = a16.outproj_case(i, fmt)
    assert torch.equal(ar.round16(c["ctx"], fmt), c["ctx"]) and torch.equal(ar.round16(c["w"], fmt), c["w"])
    assert (c["p"] > 0) == (i in a16.OUTPROJ_DROPOUT) and (c["p"] == 0 or 0.05 < 1 - c["keep"].double().mean().item() < 0.15)
    fwd = a16.outproj_fwd(c)
    f32 = a16.outproj_fwd_f32(c)
    for name in a16.OUTPROJ_OUTPUTS_FWD:                                  # sound
        r = a16.ratio(torch.from_numpy(f32[name]), *fwd[name])
        assert r <= 1.0, (name, r)
    for mname, mut in _mutations(c).items():                             # sharp
        bad = a16.outproj_fwd(c, **mut)
        for name in a16.OUTPROJ_OUTPUTS_FWD:
            r = a16.ratio(bad[name][0], *fwd[name])
            assert r >= 10.0, (name, mname, r)
    if fmt == "f16":
        return                                                            # the backward runs in math mode 2 only
    xhat, rstd = fwd["xhat"][0], fwd["rstd"][0]
    xh32, rs32 = xhat.float(), rstd.float()                               # the backward's inputs are fp32 maps: given, not derived
    for form in a16.OUTPROJ_FORMS:
        ln = a16.outproj_ln_bwd(c, form, xh32, rs32)
        pr = a16.outproj_products(c, ln["dz"][0])
        ref = {**ln, **pr}
        f32 = a16.outproj_bwd_f32(c, form, xh32.numpy(), rs32.numpy())
        # (dctx / dwfc of the restatement contract ITS OWN bf16(dz): held to the float64 products of the same operand)
        own = a16.outproj_products(c, torch.from_numpy(f32["dz"]))
        for name in a16.OUTPROJ_OUTPUTS_BWD:
            val, bound = own[name] if name in own else ref[name]
            r = a16.ratio(torch.from_numpy(f32[name]), val, bound)
            assert r <= 1.0, (form[0], name, r)
        for mname, mut in _mutations(c).items():
            bl = a16.outproj_ln_bwd(c, form, xh32, rs32, **mut)
            bp = a16.outproj_products(c, ln["dz"][0], **mut)
            for name in a16.OUTPROJ_OUTPUTS_BWD:
                r = a16.ratio({**bl, **bp}[name][0], *ref[name])
                assert r >= 10.0, (form[0], name, mname, r)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(a16.PROJECT16_SHAPES)))
def test_project16_reference(i, fmt):
    """the bound of the 16-bit projection holds for fp32 accumulation + one rounding of the result, and not for a result whose
    temperature was forgotten or reached one row too many"""
    c = a16.project16_case(i, fmt)
    assert c["div_rows"] % 4 == 0 and 0 < c["div_rows"] < c["R"]
    ref, bound = a16.project16_ref(c, fmt)
    acc = torch.einsum("rc,scn->srn", c["w"], c["x"])
    acc[:, :c["div_rows"]] /= c["temperature"]
    assert a16.ratio(ar.round16(acc, fmt), ref, bound) <= 1.0
    nodiv = torch.einsum("rc,scn->srn", c["w"], c["x"])
    assert a16.ratio(ar.round16(nodiv, fmt), ref, bound) >= 10.0           # the temperature forgotten
    acc1 = acc.clone()
    acc1[:, c["div_rows"]] /= c["temperature"]                            # one row too many divided
    assert a16.ratio(ar.round16(acc1, fmt), ref, bound) >= 10.0
