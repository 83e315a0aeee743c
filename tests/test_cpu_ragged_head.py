"""CPU-side checks (no GPU needed) of what tests/test_gpu_ragged_head.py and the weight-gradient cases of tests/test_gpu_octant.py
rest on: every closed-form backward of tests/ragged_head_ref.py equals torch autograd of the forward beside it in float64; the
input maker puts finite poison past every count and a canary in the stride padding; the case tables hold the counts, lengths and
pitches they are named for; and the weight-gradient cases of tests/octant_ref.py get the split-K chunk each is named for, read off
the library's own workspace size (a host-only call)."""
import numpy as np
import pytest
import torch

from tests import octant_ref as O
from tests import ragged_head_ref as R


def _close(a, b, rel=1e-12):
    return (a - b).abs().max().item() <= rel * max(b.abs().max().item(), 1e-300)


def _leaf(t):
    return t.double().clone().requires_grad_()


def test_pool_backward_is_autograd_of_the_pool():
    counts, C, ld = [1, 3, 4, 5, 9, 12], 5, 12
    t = R.pool_inputs(C, ld, 1, counts=counts)
    E = len(counts)
    x, gamma, beta = _leaf(R.maps(t["buf"], E, C, ld, t["stride"])), _leaf(t["gamma"]), _leaf(t["beta"])
    pooled, mean, scale = R.pool(x, counts, gamma, beta)
    assert torch.isfinite(pooled).all() and (pooled.abs() <= scale * (1 + 1e-12)).all()
    dx, dg, db = torch.autograd.grad((pooled * t["dpooled"].double()).sum(), (x, gamma, beta))
    got, g = R.pool_bwd(t["dpooled"], t["gamma"], counts, ld)
    assert _close(got, dx)
    for e, n in enumerate(counts):
        assert not dx[e, :, n:].any() and not got[e, :, n:].any() and torch.equal(got[e, :, :n], g[e][:, None].expand(C, n))
    dgamma, dbeta = R.pool_param_grads(t["dpooled"], mean.detach())
    assert _close(dgamma, dg) and _close(dbeta, db)
    prev = R.maps(t["prev"], E, C, ld, t["stride"])
    assert torch.equal(R.pool_bwd(t["dpooled"], t["gamma"], counts, ld, prev)[0], prev.double() + got)


@pytest.mark.parametrize("k1,cross_first", R.mix_layouts(3))
def test_mix_backward_is_autograd_of_the_mix(k1, cross_first):
    lens, C, ld = [1, 7, 4], 4, 8
    B = len(lens)
    t = R.mix_inputs(lens, k1, cross_first, C, ld)
    E = t["n_evals"]
    x = _leaf(R.maps(t["buf"], E, C, ld, t["stride"]))
    comp, gamma, beta = _leaf(t["comp"]), _leaf(t["gamma"]), _leaf(t["beta"])
    out, A = R.mix_fwd(x, lens, comp, gamma, beta, cross_first)
    assert out.shape == (sum(lens), C) and torch.isfinite(out).all() and (out.abs() <= A * (1 + 1e-12)).all()
    dx, dc, dg, db = torch.autograd.grad((out * t["dout"].double()).sum(), (x, comp, gamma, beta))
    b = R.mix_bwd(t["dout"], x.detach(), lens, t["comp"], t["gamma"], cross_first)
    assert _close(b["dxhat"], dx)
    mapped = sorted({R.ev(s, j, B, cross_first) for s in range(B) for j in range(k1)})
    assert b["written"].nonzero().flatten().tolist() == mapped and len(mapped) == B * k1 and mapped[-1] == E - 3
    assert not dx[~b["written"]].any()
    assert (b["rowdot"].abs() <= b["dot_abs"]).all() and (b["rowsum"].abs() <= b["sum_abs"]).all()
    dcomp, dgamma, dbeta = R.mix_param_grads(b["rowdot"], b["rowsum"], t["comp"], t["gamma"], t["beta"])
    assert _close(dcomp, dc) and _close(dgamma, dg) and _close(dbeta, db)


def test_the_evaluation_order_is_the_headers():
    assert [R.ev(b, 0, 6, 99) for b in range(6)] == list(range(6))
    assert R.ev(2, 1, 6, 9) == 11 and R.ev(2, 3, 6, 9) == 9 + 2 * 6 + 2
    # the head's own layout: X_{i,b} = B + K B + i B + b
    B, K = 3, 2
    assert [R.ev(b, j, B, B + K * B) for j in (1, 2) for b in range(B)] == list(range(B + K * B, B + 2 * K * B))
    assert R.node_counts([5, 6], [[1, 2], [3, 4]], 2) == [5, 6, 1, 2, 3, 4, 5, 6, 5, 6]


def test_the_input_maker_poisons_past_the_counts_with_finite_values():
    counts, C, ld, pad = [1, 4, 6, 8], 3, 8, 2
    buf, stride = R.make_maps(np.random.default_rng(0), counts, C, ld, pad)
    assert stride == C * ld + 4 * pad and buf.numel() == len(counts) * stride
    x = R.maps(buf, len(counts), C, ld, stride)
    assert torch.isfinite(buf).all()
    for e, n in enumerate(counts):
        assert (x[e, :, :n].abs() < 10).all()
        assert (x[e, :, n:].abs() == R.POISON).all()
        if ld - n >= 2:
            assert (x[e, :, n:].sum(dim=1).abs() <= R.POISON).all() and (x[e, 0, n] == -x[e, 0, n + 1])       # both signs
    assert (R.padding(buf, len(counts), C, ld, stride) == R.CANARY).all()
    t = R.mix_inputs([3, 5], 8, 5, 4, 8)
    assert t["comp"].abs().max() <= 2 and (t["comp"] < 0).any() and (t["comp"] > 0).any()


def test_the_case_tables_have_the_edges_they_are_named_for():
    assert {1, 3, 4, 5, 1023, 1024, 1025} <= set(R.POOL_COUNTS)
    assert R.POOL_LDS[0] == max(R.POOL_COUNTS) and R.POOL_LDS[1] >= max(R.POOL_COUNTS) + 1024       # a grid block past every count
    assert all(ld % 4 == 0 for ld in R.POOL_LDS + R.MIX_LDS)
    first, n = R.POOL_SUB
    assert 0 < first and first + n < len(R.POOL_COUNTS)
    many = R.MIX_LENS[0]
    assert {1, 63, 64, 65} <= set(many) and many[-1] < 64 and max(many) > 128
    assert len(R.MIX_LENS[1]) == 1
    for lens in R.MIX_LENS:
        assert max(lens) <= min(R.MIX_LDS)
        tiles = lambda n: (n + 63) // 64
        assert any(tiles(ld) > tiles(max(lens)) for ld in R.MIX_LDS)                # at least one tile past the longest shape
        B = len(lens)
        ks = [k1 for k1, _ in R.mix_layouts(B)]
        assert 1 in ks and 8 in ks and (3, 3 * B) in R.mix_layouts(B)
        for k1, cross_first in R.mix_layouts(B):
            if k1 > 1:
                assert cross_first >= B
            E = R.mix_n_evals(B, k1, cross_first)
            assert max(R.ev(b, j, B, cross_first) for b in range(B) for j in range(k1)) < E - 1
        k1, cross_first = R.mix_layouts(B)[-1]
        assert cross_first > B                                                      # unmixed evaluations in between
    assert any(c % 64 for c in R.MIX_CS) and any(c < 64 for c in R.MIX_CS) and any(c > 64 and c % 64 for c in R.MIX_CS)
    assert all(c % 4 == 0 for c in R.MIX_CS) and 256 in R.MIX_CS
    assert len(R.NODE_KEY_LENS) >= max(K for K, _ in R.NODE_CASES) and all(len(k) == len(R.NODE_LENS) for k in R.NODE_KEY_LENS)


def _up256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("name,c_in,c_out,chunk", O.WGRAD_CASES, ids=[f"{n}-{a}to{b}" for n, a, b, _ in O.WGRAD_CASES])
def test_the_weight_gradient_cases_get_the_chunk_they_are_named_for(name, c_in, c_out, chunk, up):
    """The workspace of the backward is the dbias partial sums up256(ceil(n_dy / 64) c_out 8) and then the slabs
    up256((ceil(n_fine / chunk) + 7) c_in c_out 4): of all chunks the rule can give (multiples of 64), only the named one fits."""
    from csn_amd import _lib
    _lib.build()
    p = O.Partition(O.WGRAD_SETS[name]())
    n_dy = p.n_fine if up else p.n_coarse
    wb = _lib.lib().csn_octant_conv_workspace_bytes(p.n_fine, p.n_coarse, c_in, c_out, int(up), 1)
    slabs = wb - _up256((n_dy + 63) // 64 * c_out * 8)
    fits = [ch for ch in range(64, 65536 + 64, 64) if _up256(((p.n_fine + ch - 1) // ch + 7) * c_in * c_out * 4) == slabs]
    assert fits == [chunk], (wb, slabs, fits)
    # a segment of this set in 16-row steps of a wave's quarter of the chunk: more than one step, which no earlier case reaches
    assert chunk // 4 > 16 and max(p.segments()) > chunk // 4


def test_the_earlier_octant_cases_stay_at_one_step_per_wave():
    """Why the cases above exist: every width of tests/test_gpu_octant.py at its largest set has chunk 64."""
    from csn_amd import _lib
    _lib.build()
    p = O.Partition(O.WGRAD_SETS["rand1031"]())
    for c_in, c_out in [(32, 32), (96, 64), (64, 96), (256, 256), (64, 64), (96, 96), (128, 128), (256, 96), (96, 256)]:
        wb = _lib.lib().csn_octant_conv_workspace_bytes(p.n_fine, p.n_coarse, c_in, c_out, 1, 1)
        slabs = wb - _up256((p.n_fine + 63) // 64 * c_out * 8)
        assert slabs == _up256(((p.n_fine + 63) // 64 + 7) * c_in * c_out * 4), (c_in, c_out)


def test_the_new_octant_sets_have_full_and_nearly_full_segments():
    assert O.Partition(O.box128()).segments() == [128] * 8
    p = O.Partition(O.box128())
    assert (p.n_fine, p.n_coarse) == (1024, 128)
    assert O.Partition(O.box127_129()).segments() == [129, 128, 128, 128, 128, 128, 128, 127]
    seg = O.Partition(O.WGRAD_SETS["rand2100"]()).segments()
    assert sum(seg) == 2100 and 192 < min(seg) and max(seg) < 2 * 192
