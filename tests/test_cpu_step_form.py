"""``csn_amd.functional.step_form``: the one decision of an attention step (which operand form, which score flow, which backward
launches), as a table of geometry + switches -> the WHOLE StepForm.  Every expectation is read off the conditions of
``_MHAEvals`` as they stood before the form object existed (scripts/trace_step_calls.py confirms them launch for launch on the
card).  No GPU: the three predicates are host functions of the library, asked under ``math_mode`` as the step asks them; the
plans live on the CPU; x_all is its shape and its requires_grad flag."""
from dataclasses import replace

import pytest

from csn_amd import functional as CF
from csn_amd import tuning
from csn_amd.csa_models import MultiHeadAttention
from csn_amd.tuning import FLASH, KEEP_SCORES, RECOMPUTE_DQ

B, K1, N = 2, 3, 10000


@pytest.fixture(scope="module", autouse=True)
def _library():
    from csn_amd import _lib
    _lib.build()


def _predicates(mode, d, T):
    """csn_attn_bwd_grouping / csn_attn_bwd_dq_no_planes_available / csn_attn_bwd_dv_scores_available under the math modes the
    step asks them in: the first and the last in the backward's, the second in the forward's"""
    L = CF._lib.lib()
    fwd = CF.forward_mode(mode, T)
    with CF.math_mode(CF.backward_mode(fwd)):
        grouping, dv_ok = L.csn_attn_bwd_grouping(d, T), L.csn_attn_bwd_dv_scores_available(d, T)
    with CF.math_mode(fwd):
        return grouping, L.csn_attn_bwd_dq_no_planes_available(d, T), dv_ok


def _form(mode, H=1, d=256, T=500, kind="csa_train", plan_b=B, x_grad=False, w_fc_shape=None, keep=True, linked=False, need_dx=None,
          monkeypatch=None):
    """step_form at config-3's geometry (one head of 256 channels, 20 blocks of 500 points) unless told otherwise, under the
    switches in force; with ``monkeypatch`` the library and the live switches are out of reach while it decides"""
    C = H * d
    att = MultiHeadAttention(H, C, d, d, block=T, n_blocks=N // T)
    plan = att.plan(kind, plan_b, 1 if kind in ("self", "cross", "qkv") else K1, "cpu")
    geo = att.geometry()
    m = CF.mode_id(mode)
    args = (tuning.current(), geo, plan, (plan.S, C, geo.n_points), w_fc_shape or (C, C), m, keep, linked, x_grad, *_predicates(m, d, T))
    if monkeypatch is not None:
        def out_of_reach(*a, **k):
            raise AssertionError("step_form is pure: no library call, no second look at the live switches")
        monkeypatch.setattr(CF._lib, "lib", out_of_reach)
        monkeypatch.setattr(tuning, "current", out_of_reach)
    try:
        return CF.step_form(*args, need_dx=need_dx)
    finally:
        if monkeypatch is not None:
            monkeypatch.undo()


# the default step of the configuration the metric is quoted on
FOLDED = CF.StepForm(mode=1, bwd_mode=1, a16=0, g16=0, operands="folded", one_pass=False, grouped_fwd=True, flow=KEEP_SCORES,
                     scores=True, sc_layout=0, pt=1, kv_f16=0, dq_grouped=True, dkv_grouped=True, dv_scores=False, ranged=None)
# ... and its unfolded form: K | V tile planes, dV from the kept scores
TILES = replace(FOLDED, operands="tiles", dv_scores=True)


def test_predicates_of_the_quoted_configuration():
    """what the rows below rest on: bf16x3 at d = 256, T = 500 has the grouped calls, the tile-major instances, the no-planes dQ
    instance and dV from the scores; bf16 has the grouped calls and the recompute flow, not the flash flow"""
    assert _predicates(1, 256, 500) == (19, 1, 1)
    grouping = _predicates(2, 256, 500)[0]
    assert grouping & 7 == 7 and not grouping & 8


def test_row01_config3_bf16x3_folds(monkeypatch):
    assert _form("bf16x3", monkeypatch=monkeypatch) == FOLDED
    assert _form("bf16x3", linked=True) == FOLDED


def test_row02_naming_a_switch_of_the_unfolded_step_unfolds():
    with tuning.override(dv_from_scores=True):
        assert _form("bf16x3") == TILES
        with tuning.override(grouped_dkv=False):
            assert _form("bf16x3") == replace(TILES, dkv_grouped=False, dv_scores=False)


def test_row03_each_condition_alone_declines_the_fold():
    assert _form("bf16x3", x_grad=True) == TILES
    # values from the slot after the keys' (plan "qkv" of one shape: v_shift = 1, one evaluation: nothing to group)
    assert _form("bf16x3", kind="qkv", plan_b=1) == replace(TILES, grouped_fwd=False)
    assert _form("bf16x3", w_fc_shape=(128, 256)) == TILES
    with tuning.override(kv_tiles=False):
        assert _form("bf16x3") == replace(TILES, operands="maps", dv_scores=False)


def test_row04_bf16_linked_runs_on_16_bit_maps():
    want = replace(TILES, mode=2, bwd_mode=2, a16=1, g16=4, flow=RECOMPUTE_DQ, scores=False, dv_scores=False)
    assert _form("bf16", linked=True) == want
    assert _form("bf16", linked=False) == replace(want, a16=0, g16=0)


def test_row05_fp16_forward_bf16_backward():
    assert _form("fp16", linked=True) == replace(TILES, mode=3, bwd_mode=2, a16=2, g16=4, flow=RECOMPUTE_DQ, scores=False,
                                                kv_f16=1, dv_scores=False)


@pytest.mark.parametrize("mode,m,d,flow", [("bf16", 2, 96, FLASH), ("bf16x3", 1, 128, RECOMPUTE_DQ), ("bf16x3", 1, 64, FLASH)],
                         ids=["row06-bf16-d96", "row07-bf16x3-d128", "row08-bf16x3-d64"])
def test_rows06_to_08_narrow_heads_take_the_configured_flow(mode, m, d, flow):
    assert _predicates(m, d, 500)[0] == 13                     # grouped dQ, recompute and flash kernels; no grouped dK / dV
    assert _form(mode, H=2, d=d) == replace(TILES, mode=m, bwd_mode=m, flow=flow, scores=False, dkv_grouped=False, dv_scores=False)


def test_row09_a_block_past_512_keys_runs_as_bf16x3_on_fp32_maps():
    want = replace(TILES, operands="maps", dv_scores=False)
    assert _form("bf16", T=600, linked=True) == want
    assert _form("fp16", T=600, linked=True) == want
    assert _form("bf16x3", T=600) == want


def test_row10_fp32():
    assert _form("fp32") == CF.StepForm(mode=0, bwd_mode=0, a16=0, g16=0, operands="maps", one_pass=False, grouped_fwd=False,
                                        flow=KEEP_SCORES, scores=True, sc_layout=0, pt=0, kv_f16=0, dq_grouped=False,
                                        dkv_grouped=False, dv_scores=False, ranged=None)


def test_row11_without_kept_scores_the_logits_path_is_the_same():
    assert _form("bf16x3", keep=False) == replace(FOLDED, scores=False)
    with tuning.override(folded_projections=False):
        assert _form("bf16x3", keep=False) == replace(TILES, scores=False)
    for mode in ("bf16", "fp16"):
        kept, free = _form(mode, linked=True), _form(mode, keep=False, linked=True)
        assert not free.scores and free.flow == KEEP_SCORES and (free.a16, free.g16) == (0, 0)      # (no backward: fp32 maps)
        assert (free.mode, free.operands, free.one_pass, free.grouped_fwd) == (kept.mode, kept.operands, kept.one_pass, kept.grouped_fwd)


def test_row12_tile_major_scores_need_the_whole_grouped_chain():
    with tuning.override(tile_major_scores=True, folded_projections=False):
        assert _form("bf16x3") == replace(TILES, sc_layout=1)
        with tuning.override(grouped_dq=False):
            assert _form("bf16x3") == replace(TILES, sc_layout=0, dq_grouped=False, dv_scores=False)
        assert _form("bf16").sc_layout == 0
    with tuning.override(tile_major_scores=True):
        assert _form("bf16x3") == replace(FOLDED, sc_layout=1)          # (still folded: the switch stays live under the fold)


def test_row13_a_plan_with_slot_ranges():
    for one_pass in (False, True):
        with tuning.override(qkv_one_pass=one_pass):
            form = _form("bf16x3", kind="cross_only")
            assert form == TILES and form.ranged is None                 # (the switch is named: unfolded; ranges: two calls)
            assert _form("bf16x3", kind="cross_only", need_dx=False) == replace(TILES, ranged=True)
            assert _form("bf16x3", kind="cross_only", x_grad=True, need_dx=True) == replace(TILES, ranged=False)
            assert _form("bf16x3", need_dx=False) == replace(TILES, one_pass=one_pass, ranged=False)
    assert _form("bf16x3", kind="cross_only") == FOLDED                  # (the fold takes slot ranges)
