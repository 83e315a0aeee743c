"""The fp16 retrieval screen without a GPU: the numpy restatement (tests/retrieval_screen_ref.py) keeps every true neighbour on
many seeds and on the engineered collections, the bound is the library's, the Python entry points refuse CPU tensors and the
switch is off by default."""
import numpy as np
import pytest
import torch

from tests import retrieval_screen_ref as ref


def _true_topk(exact, k_top):
    return torch.topk(torch.from_numpy(exact), k_top, dim=1).indices.numpy()


def _rule_keeps_every_neighbour(rows, off, C, k_top, rows2=None, off2=None):
    rows2, off2 = (rows, off) if rows2 is None else (rows2, off2)
    eps = ref.screen_eps(C)
    screen = ref.screen_scores(rows, off, rows2, off2)
    exact = ref.exact_scores(rows, off, rows2, off2)
    err = np.abs(screen - exact).max()
    assert err <= eps, (err, eps)
    keep = ref.shortlist(screen, k_top, eps)
    top = _true_topk(exact, k_top)
    assert np.take_along_axis(keep, top, axis=1).all()
    return keep, err / eps


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("C", [32, 100, 256])
def test_rule_keeps_the_float64_topk_on_many_seeds(seed, C):
    rng = np.random.default_rng(1000 * C + seed)
    make = (ref.clustered, ref.structureless, ref.near_ties)[seed % 3]
    rows, off = make(rng, 12 + seed, C)
    for k_top in (1, 2, 4, 8):
        _rule_keeps_every_neighbour(rows, off, C, k_top)


def test_clustered_collection_is_screened_to_less_than_half():
    """The input of the GPU feature test: the restatement alone re-scores well under half of the pairs."""
    rows, off = ref.clustered(np.random.default_rng(7), 32, 64)
    for k_top in (1, 2, 3, 4, 7, 8):
        keep, _ = _rule_keeps_every_neighbour(rows, off, 64, k_top)
        assert keep.sum() * 2 <= keep.size, (k_top, keep.sum(), keep.size)
    assert keep.sum(axis=1).min() >= 8


def test_near_ties_cannot_be_ordered_by_the_screen():
    rows, off = ref.near_ties(np.random.default_rng(3), 24, 64)
    keep, _ = _rule_keeps_every_neighbour(rows, off, 64, 4)
    assert keep.all()                                    # every score within 2 eps of every other: the exact pass must order them


@pytest.mark.parametrize("C", [32, 100, 256])
def test_midpoint_rows_use_most_of_the_bound_and_stay_inside(C):
    rng = np.random.default_rng(C)
    rows = ref.midpoint_rows(rng, 90, C)
    off = [0, 30, 60, 90]
    _, ratio = _rule_keeps_every_neighbour(rows, off, C, 2)
    rnd, roff = ref.structureless(np.random.default_rng(C + 1), 3, C)
    _, ratio_random = _rule_keeps_every_neighbour(rnd, roff, C, 2)
    want = ref.midpoint_expected_ratio(C)                # 0.46 at C = 32 (the completing channel holds half the norm), 0.88 at 256
    assert 0.9 * want < ratio <= 1.0 and ratio > 10 * ratio_random, (ratio, want, ratio_random)


def test_engineered_rows_stay_inside_the_bound():
    rng = np.random.default_rng(5)
    C = 256
    base, off = ref.structureless(rng, 6, C, 20, 40)
    neg = base.copy()
    neg[off[1]:off[2]] = -base[off[0]:off[0] + off[2] - off[1]] if off[2] - off[1] <= off[1] - off[0] else -base[off[1]:off[2]]
    zero = base.copy()
    zero[off[2] + 1] = 0.0
    big = base.copy()
    big[off[3]:off[4]] *= np.float32(1e20)
    big[off[4]:off[5]] *= np.float32(1e-20)
    dom = base.copy()
    dom[off[5]:off[6]] = 1e-6 * np.abs(base[off[5]:off[6]])
    dom[np.arange(off[5], off[6]), rng.integers(0, C, off[6] - off[5])] = 1.0
    for rows in (neg, zero, big, dom):
        _rule_keeps_every_neighbour(rows, off, C, 3)


def test_a_huge_key_takes_no_part_in_the_threshold():
    """A key shape scaled by 2^70 overflows the fp32 measure's sum of squares: its fp32 score is 0 while the screen, which
    rescales first, sees the true cosine.  Its screen score must not stand in for one of the K' scores that justify a drop."""
    rng = np.random.default_rng(41)
    C = 64
    q, qo = ref.structureless(rng, 6, C)
    k, ko = ref.structureless(rng, 6, C)
    k = np.concatenate([k[:ko[2]], q[qo[3]:qo[4]] * np.float32(2.0 ** 70), k[ko[3]:]])     # key 2 = query 3, huge
    ko = ko[:3] + [ko[2] + qo[4] - qo[3] + o - ko[3] for o in ko[3:]]
    screen = ref.screen_scores(q, qo, k, ko)
    fp32 = ref.fp32_scores(q, qo, k, ko)
    assert screen[3, 2] > 0.9 and fp32[3, 2] == 0.0                       # the two disagree by far more than eps ...
    wild = ref.unscreenable(k, ko)
    assert wild.tolist() == [False, False, True, False, False, False]
    eps = ref.screen_eps(C)
    for k_top in (1, 2, 3):
        top = _true_topk(fp32.astype(np.float64), k_top)
        if k_top == 1:
            assert not np.take_along_axis(ref.shortlist(screen, 1, eps), top, axis=1).all()     # ... and mislead the plain rule,
        keep = ref.shortlist(screen, k_top, eps, wild)
        assert np.take_along_axis(keep, top, axis=1).all() and keep[:, 2].all()                 # not the rule that sets it aside
    assert ref.shortlist(screen, 6, eps, wild).all()                     # fewer covered keys than K': the whole row


def test_image_has_no_subnormal_that_matters_and_pads_nothing_here():
    rows, _ = ref.structureless(np.random.default_rng(2), 2, 96, 10, 10)
    img = ref.image(rows)
    assert img.dtype == np.float16 and img.shape == rows.shape
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    sub = np.abs(img.astype(np.float64)) < 2.0 ** -14
    assert (np.abs(unit[sub]) < 2.0 ** -21 * (1 + 1e-3)).all()
    assert np.abs(img.astype(np.float64) / 2 ** ref.SHIFT - unit).max() <= 2.0 ** -11


def test_bound_is_the_library_s_and_of_the_derived_order():
    from csn_amd import _lib
    from csn_amd.minkowski_csn import screen_eps
    _lib.build()
    for C in (4, 32, 64, 96, 100, 128, 256, 288):
        assert screen_eps(C) == ref.screen_eps(C)
        assert 2.0 ** -10 < screen_eps(C) < 2.0 ** -10 + (8 * C + 600) * 2.0 ** -24


def test_switch_defaults_to_off():
    from csn_amd import tuning
    assert tuning.Tuning().retrieval_screen is False and tuning.current().retrieval_screen is False
    with tuning.override(retrieval_screen=True):
        assert tuning.current().retrieval_screen is True
    assert tuning.current().retrieval_screen is False


def test_entry_points_refuse_cpu_tensors():
    from csn_amd import CsnError
    from csn_amd import minkowski_csn as M
    f, off = torch.zeros(8, 32), [0, 3, 8]
    with pytest.raises(CsnError, match="no CPU path"):
        M.retrieval_screen_ragged(f, off, f, off)
    with pytest.raises(CsnError, match="no CPU path"):
        M.retrieval_pairs_ragged(f, off, f, off, torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(CsnError, match="no CPU path"):
        M.topk_retrieval_ragged(f, off, f, off, 1, True)
    with pytest.raises(CsnError, match="no CPU path"):
        M.knn_graph_screened(f.reshape(2, 4, 32), f.reshape(2, 4, 32), 1)


def test_bad_arguments_are_rejected_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert L.csn_ragged_retrieval_screen_f16(None, None, None, 1, None, None, None, 1, 32, None, None, 0, None) == -1
    assert L.csn_ragged_retrieval_pairs_f32(None, None, None, 1, None, None, None, 1, 32, None, 1, None, None, 0, None) == -1
    assert L.csn_retrieval_screen_workspace_floats(10, 20, 2, 3, 7, 100) == 30 * 64 + 6
    assert L.csn_retrieval_screen_eps(0) == 0.0
