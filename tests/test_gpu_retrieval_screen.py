"""The fp16 retrieval screen on the MI355X: the screen kernel against float64 inside the DERIVED bound at every edge of its loops,
the pair-list kernel bit for bit against the all-pairs one, and the feature — top-K neighbours through the screen equal to
the all-pairs fp32 path as lists of integers, for the MinkowskiNet head's shape graph and for MID-FC's kNN graphs.

Worst |screen - float64| / eps seen by the bound tests on the MI355X (each test prints its own; DESIGN.md "fp16 screen of the
shape graph" keeps the figures): shape grid 0.153 (C = 32), 0.032 (96), 0.049 (100), 0.017 (256); engineered rows 0.036; rows just
under fp16 rounding midpoints 0.865 at C = 256 (0.438 at C = 32) against 0.005 (0.015) on random rows of the same geometry."""
import os

import numpy as np
import pytest
import torch

from tests import retrieval_screen_ref as ref

pytestmark = pytest.mark.gpu

N1 = [1, 127, 128, 129, 300]                 # query shapes: below / at / past the 128-point work-group tile, three tiles
N2 = [1, 5, 128, 131, 257, 64, 65]           # key shapes: the 64-point candidate tile's edges, one to five tiles


@pytest.fixture(scope="module")
def M():
    from csn_amd import _lib
    from csn_amd import minkowski_csn as m
    _lib.build()
    return m


def _offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _check_bound(M, f1, o1, f2, o2, C, what):
    got = M.retrieval_screen_ragged(_dev(f1), o1, _dev(f2), o2)
    assert torch.equal(got, M.retrieval_screen_ragged(_dev(f1), o1, _dev(f2), o2))          # no atomics: the same bits
    got = got.cpu().numpy().astype(np.float64)
    eps = ref.screen_eps(C)
    ratio = np.abs(got - ref.exact_scores(f1, o1, f2, o2)).max() / eps
    same_operands = np.abs(got - ref.screen_scores(f1, o1, f2, o2)).max()
    print(f"screen {what} C={C}: max|r16 - r64| / eps = {ratio:.4f} (eps {eps:.3e}); against the restatement's operands "
          f"{same_operands:.2e} (accumulation term {ref.accumulation_tolerance(C):.2e})")
    assert ratio <= 1.0
    assert same_operands <= ref.accumulation_tolerance(C)
    return ratio


@pytest.mark.parametrize("C", [32, 96, 100, 256])
def test_screen_against_float64_on_the_shape_grid(M, C):
    rng = np.random.default_rng(C)
    o1, o2 = _offsets(N1), _offsets(N2)
    centre = rng.standard_normal((1, C))
    f1 = (rng.standard_normal((o1[-1], C)) + 0.5 * centre).astype(np.float32)
    f2 = (rng.standard_normal((o2[-1], C)) + 0.5 * centre).astype(np.float32)
    _check_bound(M, f1, o1, f2, o2, C, "grid")


def test_screen_engineered_rows(M):
    C = 256
    rng = np.random.default_rng(77)
    o1, o2 = _offsets(N1), _offsets(N2)
    f1 = rng.standard_normal((o1[-1], C)).astype(np.float32)
    f2 = rng.standard_normal((o2[-1], C)).astype(np.float32)
    centre = 4.0 * rng.standard_normal((1, C))               # a tight shape and two negated ones: every cosine negative,
    f1[o1[3]:o1[4]] = centre + 0.2 * rng.standard_normal((N1[3], C))
    f2[o2[3]:o2[4]] = -(centre + 0.2 * rng.standard_normal((N2[3], C)))
    f2[o2[1]:o2[2]] = -(centre + 0.2 * rng.standard_normal((N2[1], C)))     # ... 5 points and 59 rows of padding that must not win
    f1[o1[4] + 7] = 0.0                                      # all-zero rows on both sides
    f2[o2[4] + 100] = 0.0
    f1[o1[1]:o1[2]] *= np.float32(1e20)
    f2[o2[2]:o2[3]] *= np.float32(1e-20)
    f2[o2[5]:o2[6]] *= np.float32(1e20)
    dom = 1e-6 * np.abs(rng.standard_normal((N2[6], C)))     # one dominant channel, 255 channels 1e-6 below it
    dom[np.arange(N2[6]), rng.integers(0, C, N2[6])] = 1.0
    f2[o2[6]:o2[7]] = dom
    f1[o1[2]:o1[2] + 64] = dom[:64]
    _check_bound(M, f1, o1, f2, o2, C, "engineered")
    got = M.retrieval_screen_ragged(_dev(f1), o1, _dev(f2), o2).cpu().numpy()
    assert got[3, 3] < -0.9 and got[3, 1] < -0.9             # the negated shapes score negative: zero padding never won


@pytest.mark.parametrize("C", [32, 256])
def test_screen_midpoint_rows_reach_the_bound_s_order(M, C):
    rng = np.random.default_rng(C + 5)
    rows = ref.midpoint_rows(rng, 300, C)
    off = [0, 70, 199, 300]
    ratio = _check_bound(M, rows, off, rows, off, C, "midpoints")
    rnd = rng.standard_normal((300, C)).astype(np.float32)
    ratio_random = _check_bound(M, rnd, off, rnd, off, C, "random")
    want = ref.midpoint_expected_ratio(C)
    assert ratio > 0.9 * want and ratio > 10 * ratio_random, (ratio, want, ratio_random)


def test_screen_refuses_what_its_images_cannot_hold(M):
    from csn_amd import CsnError
    f = torch.zeros(8, 320, device="cuda")
    with pytest.raises(CsnError, match="288"):
        M.retrieval_screen_ragged(f, [0, 8], f, [0, 8])


def test_pair_list_equals_the_all_pairs_entries(M):
    rng = np.random.default_rng(31)
    C = 100
    o1, o2 = _offsets(N1), _offsets([1, 5, 128, 131, 257])
    f1, f2 = _dev(rng.standard_normal((o1[-1], C))), _dev(rng.standard_normal((o2[-1], C)))
    full = M.retrieval_measure_ragged(f1, o1, f2, o2)
    S1, S2 = full.shape
    every = torch.cartesian_prod(torch.arange(S1), torch.arange(S2))
    lists = [torch.tensor([[3, 2]]), every, every[torch.randperm(S1 * S2, generator=torch.Generator().manual_seed(1))],
             torch.from_numpy(np.stack([rng.integers(0, S1, 60), rng.integers(0, S2, 60)], axis=1))]       # repeats, any order
    for pairs in lists:
        for dtype in (torch.int32, torch.int64):
            p = pairs.to(dtype).cuda()
            got = M.retrieval_pairs_ragged(f1, o1, f2, o2, p)
            assert torch.equal(got, full[p[:, 0].long(), p[:, 1].long()])
    assert torch.equal(M.retrieval_pairs_ragged(f1, o1, f2, o2, lists[3].cuda(), pair_budget=7),
                       full[lists[3][:, 0].cuda(), lists[3][:, 1].cuda()])
    outside = M.retrieval_pairs_ragged(f1, o1, f2, o2, torch.tensor([[0, 0], [S1, 0], [0, -1]]).cuda())
    assert outside[0] == full[0, 0] and torch.isnan(outside[1:]).all()      # not a pair: nothing read, nan written


# ---- the feature ------------------------------------------------------------------------------------------------------------
def _collections():
    C = 64
    out = {"clustered": ref.clustered(np.random.default_rng(7), 32, C),            # (test_cpu_retrieval_screen: < half re-scored)
           "clustered40": ref.clustered(np.random.default_rng(8), 40, C, lo=1, hi=300),
           "structureless": ref.structureless(np.random.default_rng(9), 24, C),
           "near_ties": ref.near_ties(np.random.default_rng(3), 24, C)}
    rows, off = ref.clustered(np.random.default_rng(10), 24, C)
    rows = rows.copy()
    rows[off[5] + 3, 11] = np.nan
    out["nan_row"] = (rows, off)
    return out


@pytest.fixture(scope="module")
def exact(M):
    """The all-pairs fp32 scores of every collection against itself, once."""
    cols = _collections()
    return {name: (rows, off, M.retrieval_measure_ragged(_dev(rows), off, _dev(rows), off).cpu()) for name, (rows, off) in cols.items()}


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("is_same", [True, False])
@pytest.mark.parametrize("name", ["clustered", "clustered40", "structureless", "near_ties", "nan_row"])
def test_topk_through_the_screen_is_the_all_pairs_topk(M, exact, name, is_same, K):
    rows, off, sim = exact[name]
    f = _dev(rows)
    got, stats = M.topk_retrieval_ragged(f, off, f, off, K, is_same)
    assert got == M.topk_neighbors(sim, K, is_same)
    S = len(off) - 1
    assert stats["pairs_screened"] == S * S and K <= stats["max_shortlist"] <= S
    print(f"{name} K={K} is_same={is_same}: {stats}")
    if name == "clustered":
        assert stats["pairs_rescored"] * 2 <= stats["pairs_screened"]        # the screen screened: at most half re-scored
    if name == "near_ties":
        assert stats["pairs_rescored"] == S * S                             # it cannot order them: the exact pass does


def _with_huge(rows, off, whole_shape, one_point):
    """A copy with shape ``whole_shape`` scaled by 2^70 and one point of shape ``one_point`` by 2^60: beyond 2^55 the fp32 measure's
    sums of squares overflow (its cosines with those rows are 0) while the screen, which rescales first, sees the true cosines."""
    rows = rows.copy()
    rows[off[whole_shape]:off[whole_shape + 1]] *= np.float32(2.0 ** 70)
    rows[off[one_point] + 1] *= np.float32(2.0 ** 60)
    return rows


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("is_same", [True, False])
def test_topk_with_shapes_the_bound_does_not_cover(M, is_same, K):
    """Huge shapes are scored in full as queries, always scored as keys and kept out of every row's threshold: the neighbours
    are those of the all-pairs path, where those keys score ~0 — far from their screen scores."""
    rows, off = ref.clustered(np.random.default_rng(21), 24, 64)
    f = _dev(_with_huge(rows, off, 4, 9))                    # (families of 4: shapes 0, 4, 8, ... and 1, 5, 9, ... score ~1 in real arithmetic)
    q, qoff = (f, off) if is_same else (_dev(rows), off)     # not the same set: clean queries against the keys with huge shapes
    sim = M.retrieval_measure_ragged(q, qoff, f, off).cpu()
    screen = M.retrieval_screen_ragged(q, qoff, f, off).cpu()
    assert (screen[0, 4] - sim[0, 4]).abs() > 0.3            # the premise: screen and fp32 disagree on the huge key
    got, stats = M.topk_retrieval_ragged(q, qoff, f, off, K, is_same)
    assert got == M.topk_neighbors(sim, K, is_same)
    assert stats["pairs_rescored"] < stats["pairs_screened"]


@pytest.mark.parametrize("same", [True, False])
def test_knn_graph_screened_with_shapes_the_bound_does_not_cover(M, same):
    from csn_amd import functional as CF
    rng = np.random.default_rng(22)
    S, N, C, K = 12, 150, 64, 2
    rows, off = ref.clustered(rng, S, C, lo=N, hi=N)
    huge = _dev(_with_huge(rows, off, 4, 9)).reshape(S, N, C)
    q = huge if same else _dev(rows).reshape(S, N, C)
    want = CF.retrieval_measure(q, huge).topk(K + 1, -1)[1]
    got, stats = M.knn_graph_screened(q, huge, K)
    assert torch.equal(got, want) and stats["pairs_rescored"] < stats["pairs_screened"]


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("is_same", [True, False])
def test_topk_minimum_key_set_and_row_chunks(M, exact, is_same, K):
    rows, off, sim = exact["clustered"]
    k_top = K + 1 if is_same else K
    f = _dev(rows)
    koff = off[:k_top + 1]                                   # S_k = K': every key is a neighbour
    got, stats = M.topk_retrieval_ragged(f, off, f[:koff[-1]], koff, K, is_same)
    assert got == M.topk_neighbors(sim[:, :k_top], K, is_same) and stats["pairs_rescored"] == stats["pairs_screened"]
    chunked, cstats = M.topk_retrieval_ragged(f, off, f, off, K, is_same, pair_budget=100)       # three query rows per chunk
    assert chunked == M.topk_neighbors(sim, K, is_same)
    assert cstats["pairs_rescored"] == M.topk_retrieval_ragged(f, off, f, off, K, is_same)[1]["pairs_rescored"]
    if k_top > 1:                                            # fewer keys than K': today's path, today's error
        with pytest.raises(RuntimeError):
            M.topk_neighbors(sim[:, :k_top - 1], K, is_same)
        with pytest.raises(RuntimeError):
            M.topk_retrieval_ragged(f, off, f[:off[k_top - 1]], off[:k_top], K, is_same)


@pytest.mark.parametrize("is_same", [True, False])
def test_shape_graph_with_and_without_the_screen(M, is_same):
    from csn_amd import tuning
    torch.manual_seed(4)
    C, K = 64, 3
    head = M.SimCSNHead(C, 2, 5, K).cuda().eval()
    rows, off = ref.clustered(np.random.default_rng(12), 24, C)
    shapes = [_dev(rows[a:b]) for a, b in zip(off, off[1:])]
    keys = None if is_same else shapes[:9]
    want = M.construct_shape_graph(head, shapes, keys, K=K, max_rows=500, screen=False)
    assert M.construct_shape_graph(head, shapes, keys, K=K, max_rows=500) == want            # the switch is off
    assert M.construct_shape_graph(head, shapes, keys, K=K, max_rows=500, screen=True) == want
    with tuning.override(retrieval_screen=True):
        assert M.construct_shape_graph(head, shapes, keys, K=K, max_rows=500) == want
        assert M.construct_shape_graph(head, shapes, keys, K=K, max_rows=500, screen=False) == want


# ---- MID-FC -----------------------------------------------------------------------------------------------------------------
def test_g6_knn_graph_through_the_screen(M, golden_dir):
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    from oracle import csa_oracle as orc
    g = np.load(os.path.join(golden_dir, "g6_retrieval.npz"))
    model = get_model("ssa", 4, 1).cuda().eval()
    for i in range(2):
        S, N, K, seed = (int(v) for v in g[f"g6_{i}_cfg"])
        f = orc.synth_clustered_feats(np.random.default_rng(seed), S, N)
        with tuning.override(retrieval_screen=True):
            graph = model.get_knn_graph(f, f, K).cpu()
        assert graph.dtype == torch.int64 and graph.shape == (S, K + 1)
        assert np.array_equal(graph.numpy(), g[f"g6_{i}_graph"])
        idx, stats = M.knn_graph_screened(f.cuda(), f.cuda(), K)
        print(f"g6_{i}: {stats}")
        assert torch.equal(idx.cpu(), graph) and stats["pairs_rescored"] < stats["pairs_screened"]


def test_knn_graph_big_with_and_without_the_screen(M):
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    from oracle import csa_oracle as orc
    torch.manual_seed(2)
    rng = np.random.default_rng(15)
    K = 2
    model = get_model("ssa", 4, 1).cuda().eval()
    lab = torch.zeros((1, 10000), dtype=torch.int64)
    train = [(x.cuda(), lab) for x in orc.synth_clustered_shapes(rng, 9, 3)]
    test = [(x.cuda(), lab) for x in orc.synth_clustered_shapes(rng, 4, 3)]
    centres = np.array([0, 1, 2, 4, 5, 8])
    want = [model.get_knn_graph_big(q, train, centres.copy(), K).cpu() for q in (train, test)]
    with tuning.override(retrieval_screen=True):
        got = [model.get_knn_graph_big(q, train, centres.copy(), K).cpu() for q in (train, test)]
    for a, b in zip(got, want):
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a, b)
