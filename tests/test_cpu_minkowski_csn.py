"""CPU-side checks of the MinkowskiNet cross-shape head (csn_amd/minkowski_csn.py, include/csn_hip.h section 11): the new entry
points reject bad arguments on the host before anything is enqueued, the module's parameters mirror hrnet.py:341-357, and the
host-side pieces of the shape graph (batch offsets, the top-K rule of csn_utils.py:91-96, the random branch of :31-43) behave
as the reference does.  No compute call is made here."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 4096          # a non-null, 16-byte aligned "device pointer": every call below must be rejected before it is used


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib.lib()


def _ints(*v):
    a = (ctypes.c_int * len(v))(*v)
    return ctypes.cast(a, ctypes.c_void_p).value, a


def test_ragged_pool_rejects_bad_arguments(L):
    good, _g = _ints(5, 8)
    bad, _b = _ints(5, 9)               # a count beyond ld = 8
    zero, _z = _ints(0, 3)
    ok = dict(xhat=FAKE, es=256 * 8, ld=8, ch=good, cd=FAKE, n=2, c=256)
    def pool(**kw):
        a = {**ok, **kw}
        return L.csn_ragged_pool_f32(a["xhat"], a["es"], a["ld"], a["ch"], a["cd"], a["n"], a["c"], FAKE, FAKE, FAKE, None, None)
    assert pool(xhat=None) == -1
    assert pool(ch=None) == -1
    assert pool(cd=None) == -1
    assert pool(ch=bad) == -1
    assert pool(ch=zero) == -1
    assert pool(n=0) == -1
    assert pool(es=256 * 8 - 4) == -1   # an evaluation stride shorter than its maps
    assert L.csn_ragged_pool_bwd_f32(FAKE, FAKE, good, FAKE, 2, 256, FAKE, 256 * 8, 8, 2, None) == -1      # accumulate flag
    assert L.csn_ragged_pool_bwd_f32(FAKE, FAKE, bad, FAKE, 2, 256, FAKE, 256 * 8, 8, 0, None) == -1
    assert L.csn_ragged_pool_bwd_f32(None, FAKE, good, FAKE, 2, 256, FAKE, 256 * 8, 8, 0, None) == -1


def test_ragged_mix_rejects_bad_arguments(L):
    off, _o = _ints(0, 5, 12, 13)
    nonmono, _n = _ints(0, 5, 5, 13)     # an empty shape
    down, _d = _ints(0, 7, 3, 13)        # decreasing
    start, _s = _ints(1, 5, 12, 13)      # not starting at 0
    longer, _l = _ints(0, 5, 30, 31)     # a shape longer than ld
    C, ld, E = 256, 12, 9                # B = 3, K = 2: S 0..2, T 3..8 ... cross_first = 9 needs E >= 15
    def fwd(offh=off, n_evals=15, cross_first=9, k1=3, ld_=ld, ld_out=2 * C, ch=C):
        return L.csn_ragged_mix_fwd_f32(FAKE, C * ld, ld_, n_evals, cross_first, offh, FAKE, 3, k1, ch, FAKE, FAKE, FAKE, FAKE,
                                        ld_out, None)
    def bwd(offh=off, n_evals=15, cross_first=9, k1=3, ws=10 ** 9, rowdot=FAKE):
        return L.csn_ragged_mix_bwd_f32(FAKE, 2 * C, FAKE, C * ld, ld, n_evals, cross_first, offh, FAKE, 3, k1, C, FAKE, FAKE,
                                        FAKE, rowdot, FAKE, FAKE, ws, None)
    for f in (fwd, bwd):
        assert f(offh=None) == -1
        assert f(offh=nonmono) == -1
        assert f(offh=down) == -1
        assert f(offh=start) == -1
        assert f(offh=longer) == -1
        assert f(n_evals=E) == -1            # the cross evaluations would run past the maps
        assert f(cross_first=1) == -1        # cross evaluations overlapping the shapes' own
        assert f(k1=9) == -1
        assert f(k1=0) == -1
    assert fwd(ld_out=C - 4) == -1
    assert bwd(rowdot=None) == -1
    assert bwd(ws=1) == -6                   # workspace too small (still before any launch)


def test_ragged_retrieval_rejects_bad_arguments(L):
    o1, _a = _ints(0, 3, 10)
    o2, _b = _ints(0, 4)
    bad, _c = _ints(0, 6, 2)
    def call(h1=o1, h2=o2, s1=2, s2=1, c=256, out=FAKE, ws_n=10 ** 9):
        return L.csn_ragged_retrieval_f32(FAKE, h1, FAKE, s1, FAKE, h2, FAKE, s2, c, out, FAKE, ws_n, None)
    assert call(h1=None) == -1
    assert call(h2=None) == -1
    assert call(h1=bad) == -1
    assert call(s1=0) == -1
    assert call(out=None) == -1
    assert call(c=0) == -1
    assert call(ws_n=10) == -6


def test_state_dict_mirrors_hrnet():
    from csn_amd.minkowski_csn import SimCSNHead
    h = SimCSNHead(256, 4, 13, k_neighbors=2)
    shapes = {k: tuple(v.shape) for k, v in h.state_dict().items()}
    assert shapes == {
        "MHA.w_qs.weight": (256, 256), "MHA.w_ks.weight": (256, 256), "MHA.w_vs.weight": (256, 256),
        "MHA.fc.weight": (256, 256), "MHA.norm.weight": (256,), "MHA.norm.bias": (256,),
        "output.weight": (13, 512), "output.bias": (13,),
        "linear_q.weight": (256, 256), "linear_k.weight": (256, 256)}
    assert h.sim.temperature == 16.0
    h0 = SimCSNHead(128, 4, 7, k_neighbors=0)
    assert not any(k.startswith("linear_") for k in h0.state_dict())
    assert not hasattr(h0, "sim") and not hasattr(h0, "linear_q")
    # n_head 3 at 256: d_k = 85, as hrnet.py:343 builds it
    assert tuple(SimCSNHead(256, 3, 5, 1).state_dict()["MHA.w_qs.weight"].shape) == (255, 256)


def test_unsupported_width_and_cpu_tensors_are_refused():
    from csn_amd import _lib
    from csn_amd.minkowski_csn import SimCSNHead
    with pytest.raises(ValueError, match="LayerNorm"):
        SimCSNHead(200, 4, 5, 1)
    h = SimCSNHead(64, 2, 5, 1)
    with pytest.raises(_lib.CsnError):
        h(torch.zeros(10, 64), [0, 4, 10])


def test_offsets_from_batch_index():
    from csn_amd.minkowski_csn import offsets_from_batch_index
    assert offsets_from_batch_index(torch.tensor([0, 0, 0, 1, 2, 2])).tolist() == [0, 3, 4, 6]
    assert offsets_from_batch_index(np.array([0])).tolist() == [0, 1]
    with pytest.raises(ValueError, match="sorted"):
        offsets_from_batch_index(torch.tensor([0, 1, 0, 1]))
    with pytest.raises(ValueError):
        offsets_from_batch_index(torch.tensor([0, 0, 2]))           # shape 1 has no rows
    with pytest.raises(ValueError):
        offsets_from_batch_index(torch.tensor([0, 1]), n_shapes=3)


def _reference_rule(sim, K, is_same):
    """csn_utils.py:91-96, restated row by row."""
    out = []
    for q in range(sim.shape[0]):
        vals, idx = torch.topk(sim[q], K)
        if is_same and q in idx:
            vals, idx = torch.topk(sim[q], K + 1)
            idx = idx[q != idx]
        out.append((q, idx.tolist()))
    return out


def test_topk_rule_by_hand():
    from csn_amd.minkowski_csn import topk_neighbors
    sim = torch.tensor([[1.0, 0.2, 0.7, 0.4],       # self first: dropped, the next two
                        [0.9, 0.1, 0.8, 0.3],       # self last: plain top 2
                        [0.5, 0.6, 0.95, 0.7],      # self first
                        [0.3, 0.9, 0.2, 0.85]])     # self second
    got = topk_neighbors(sim, 2, True)
    assert got == [(0, [2, 3]), (1, [0, 2]), (2, [3, 1]), (3, [1, 0])]
    assert got == _reference_rule(sim, 2, True)
    assert topk_neighbors(sim, 1, True) == [(0, [2]), (1, [0]), (2, [3]), (3, [1])]
    # key_shapes given: the query index names ANOTHER set, nothing is dropped
    assert topk_neighbors(sim, 2, False) == [(0, [0, 2]), (1, [0, 2]), (2, [2, 3]), (3, [1, 3])]
    rect = torch.tensor([[0.1, 0.5, 0.3], [0.7, 0.2, 0.6]])
    assert topk_neighbors(rect, 2, False) == [(0, [1, 2]), (1, [0, 2])] == _reference_rule(rect, 2, False)


def test_random_branch():
    from csn_amd.minkowski_csn import construct_shape_graph, random_neighbors
    shapes = [None] * 9                                  # the random branch never looks at the features
    a = construct_shape_graph(None, shapes, K=3, random_pairs=True, rng=np.random.default_rng(5))
    b = construct_shape_graph(None, shapes, K=3, random_pairs=True, rng=np.random.default_rng(5))
    assert a == b
    assert [q for q, _ in a] == list(range(9))
    for q, nb in a:
        assert len(nb) == 3 and len(set(nb)) == 3 and q not in nb and all(0 <= i < 9 for i in nb)
    # with key shapes: the query index may appear (another set), still K distinct
    c = random_neighbors(4, 5, 5, False, np.random.default_rng(1))
    assert all(sorted(nb) == [0, 1, 2, 3, 4] for _, nb in c)
    with pytest.raises(ValueError):
        random_neighbors(4, 4, 4, True, np.random.default_rng(1))
    with pytest.raises(ValueError):
        construct_shape_graph(None, shapes, K=1, random_pairs=True)
