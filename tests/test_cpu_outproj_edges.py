"""The derived bounds of tests/outproj_edge_ref.py (out-projection + LayerNorm in math modes 0 and 1), checked without a GPU on
every case of the GPU file: SOUND for the arithmetic they describe (a float32 restatement — plain fp32 in mode 0, both operands
split as split4 does and the three products accumulated in fp32 in mode 1 — stays under them) and SHARP (a point, a channel row or
the last four points dropped on float64 data moves every output to at least 10x its bound)."""
import pytest
import torch

from tests import act16_ref as a16
from tests import outproj_edge_ref as oe

K = range(len(oe.CASES))


def test_the_cases_are_the_issues():
    ten = a16.OUTPROJ_SHAPES
    for m in (0, 1):
        got = [(c[1:5], c[6]) for c in oe.CASES if c[0] == m][:len(ten)]
        assert got == [(s, 0.1 if i in a16.OUTPROJ_DROPOUT else 0.0) for i, s in enumerate(ten)]
    assert [c for c in oe.CASES[2 * len(ten):]] == [(1, 256, 256, 4, 4, 3, 0.0), (1, 256, 256, 36, 40, 3, 0.0),
                                                    (1, 256, 256, 252, 256, 3, 0.1), (1, 256, 256, 260, 264, 40, 0.1)]
    assert len({oe.case_id(k) for k in K}) == len(oe.CASES)
    assert oe.forms(a16.E_OUT) == a16.OUTPROJ_FORMS


def test_the_ten_shapes_keep_their_act16_values_before_rounding():
    """the same draws as a16.outproj_case, not rounded: rounding them gives the act16 case (Ctx up to its flush)"""
    for k in (1, 14):
        c, b = oe.case(k), a16.outproj_case(oe.SEED_INDEX[k], "bf16")
        assert torch.equal(c["w"].bfloat16().float(), b["w"]) and torch.equal(c["dxhat"].bfloat16().float(), b["dxhat"])
        assert torch.equal(a16.flush_f16(c["ctx"].bfloat16().float()), b["ctx"]) and torch.equal(c["x"], b["x"])
        assert torch.equal(c["keep"], b["keep"]) and c["seed"] == b["seed"] and c["res_index"] == a16.RES_INDEX
        assert not torch.equal(c["w"].bfloat16().float(), c["w"])          # full fp32 operands


def test_split_is_split4():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(3)).numpy()
    hi, lo = oe.split(v)
    u = oe.U_BF16
    assert (abs(v - hi) <= u * abs(v)).all() and (abs(v - hi - lo) <= u * u * abs(v)).all()
    assert torch.equal(torch.from_numpy(hi).bfloat16().float(), torch.from_numpy(hi))
    assert torch.equal(torch.from_numpy(lo).bfloat16().float(), torch.from_numpy(lo))
    # the dropped terms against the derived 3 u^2 (1 + u) |a b|, product by product
    w = torch.randn(4096, generator=torch.Generator().manual_seed(4)).numpy()
    wh, wl = oe.split(w)
    three = wl.astype("f8") * hi + wh.astype("f8") * lo + wh.astype("f8") * hi
    assert (abs(v.astype("f8") * w - three) <= 3 * u * u * (1 + u) * abs(v.astype("f8") * w)).all()


@pytest.mark.parametrize("k", K, ids=[oe.case_id(k) for k in K])
def test_outproj_bounds_are_sharp_and_sound(k):
    c = oe.case(k)
    assert c["p"] == oe.CASES[k][6] and (c["p"] == 0 or 0.05 < oe.dropped_fraction(c) < 0.15)
    fwd = oe.fwd(c)
    f32 = oe.fwd_f32(c)
    for name in a16.OUTPROJ_OUTPUTS_FWD:                                  # sound
        r = a16.ratio(torch.from_numpy(f32[name]), *fwd[name])
        assert r <= 1.0, (name, r)
    for mname, mut in oe.mutations(c).items():                           # sharp
        bad = oe.fwd(c, **mut)
        for name in a16.OUTPROJ_OUTPUTS_FWD:
            r = a16.ratio(bad[name][0], *fwd[name])
            assert r >= 10.0, (name, mname, r)
    xh32, rs32 = fwd["xhat"][0].float(), fwd["rstd"][0].float()           # the backward's inputs are fp32 maps: given, not derived
    for form in oe.forms(c["E"]):
        ln = oe.ln_bwd(c, form, xh32, rs32)
        pr = oe.products(c, ln["dz"][0].float())
        ref = {**ln, **pr}
        f32 = oe.bwd_f32(c, form, xh32.numpy(), rs32.numpy())
        # (dctx / dwfc of the restatement contract ITS OWN dz: held to the float64 products of the same operand)
        own = oe.products(c, torch.from_numpy(f32["dz"]))
        for name in a16.OUTPROJ_OUTPUTS_BWD:
            val, bound = own[name] if name in own else ref[name]
            r = a16.ratio(torch.from_numpy(f32[name]), val, bound)
            assert r <= 1.0, (form[0], name, r)
        for mname, mut in oe.mutations(c).items():
            bl = oe.ln_bwd(c, form, xh32, rs32, **mut)
            bp = oe.products(c, ln["dz"][0].float(), **mut)
            for name in a16.OUTPROJ_OUTPUTS_BWD:
                r = a16.ratio({**bl, **bp}[name][0], *ref[name])
                assert r >= 10.0, (form[0], name, mname, r)
