"""GPU checks of the four entry points of include/csn_hip.h section 28 (csn_amd/csrc/train_maps16.hip: the HRNet backbone's training
launches on bf16 activation maps), one call at a time through the raw C ABI, in math mode 2 with the single-product instances selected.

The contract is exactness: a bf16 map changes where a value is stored, not which product or sum is formed.  Every comparison is
``torch.equal`` (or equal bits) against the fp32 entry point fed the same values as fp32.

(28a) + (28d), ``csn_sparse_conv_stats_fwd_t16`` / ``csn_sparse_conv_bwd_t16``: kernel-27 stride-1 maps of 2, 31, 33, 64, 65, 127, 129
and 257 rows (either side of the 32-row wave tile, the 64-row split-K chunk — 65, 129 and 257 leave a partial last chunk — and the
128-row work-group tile), the stride-2 map and its transposed form, and a set whose last tiles hold isolated voxels (offsets without
a neighbour: dropped offsets forward, skipped 16-row steps in the weight gradient), at the widths (32, 32), (64, 128), (96, 96) and
(256, 256), which take TA = 1, 2, 3 and 4 in the weight gradient; every column-block count pinned through ``CSN_DEV_SCONV_NB``.
Compared: z, mean, invstd, the running statistics, dW (and dx, which section 28 leaves to section 14).

(28b) + (28c), ``csn_rows_bn_act_fwd_t16`` / ``_bwd_t16``: 1, 63, 64, 65 and 129 rows (either side of the 64-row chunk), 32, 96 (16 idle
threads) and 256 columns, 1 to 3 terms, no residual / a bf16 residual, ReLU on and off, y bf16 and fp32, plus a map of hand-picked
values: exact zeros, -0, values that round to -0 and ties.  Compared: y as the bits of the fp32 result rounded once (torch's cast);
dz per term, dgamma, dbeta and dr against the fp32 backward on the widened y."""
import ctypes
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R
from tests.test_gpu_hrnet import TWO_ROWS, bn_act_case

pytestmark = pytest.mark.gpu

WIDTHS = [(32, 32), (64, 128), (96, 96), (256, 256)]
SIZES = [2, 31, 33, 64, 65, 127, 129, 257]
STRIDED = [33, 129, 257]


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def bf16_single_product(L):
    from csn_amd import functional as CF
    with CF.math_mode(2), CF.rows16(True):
        yield


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------
# (28a) convolution + statistics, (28d) weight gradient
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kmap(kind, name):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = TWO_ROWS if name == 2 else (R.two_clusters() if name == "clusters" else R.random_set(name))
    pts = torch.tensor(pts)
    if kind == "s1":
        return build_kernel_map(pts, kernel_size=3).to("cuda")
    m = build_kernel_map(pts, kernel_size=3, stride=2)
    return (m if kind == "s2" else m.transpose()).to("cuda")


def _conv_both(L, m, c_in, c_out, seed):
    """The fp32 entry points on the widened values and section 28 on the bf16 rows: (z, mean, invstd, rm, rv, dx, dw) of each."""
    lib = L.lib()
    g = torch.Generator().manual_seed(seed)
    x16 = torch.randn(m.n_in, c_in, generator=g).cuda().bfloat16()
    w = (torch.randn(m.KV, c_in, c_out, generator=g) / (m.KV * c_in) ** 0.5).cuda()
    dy = torch.randn(m.n_out, c_out, generator=g).cuda()
    rm0, rv0 = 0.1 * torch.randn(c_out, generator=g), 1 + 0.1 * torch.randn(c_out, generator=g).abs()
    wb = lib.csn_sparse_conv_stats_workspace_bytes(m.n_out, c_out)
    bb = lib.csn_sparse_conv_workspace_bytes(m.n_in, m.n_out, m.KV, c_in, c_out, 1)
    outs = []
    for new in (False, True):
        x = x16 if new else x16.float()
        z, dx, dw = torch.empty(m.n_out, c_out, device="cuda"), torch.empty(m.n_in, c_in, device="cuda"), torch.empty_like(w)
        mean, invstd, rm, rv = torch.empty(c_out, device="cuda"), torch.empty(c_out, device="cuda"), rm0.cuda(), rv0.cuda()
        ws = torch.empty(max(wb, bb, 16), dtype=torch.uint8, device="cuda")
        tail = (m.n_in, _ptr(m.fwd), m.n_out, m.KV, c_in, c_out, _ptr(w), _ptr(z), c_out, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv),
                H.EPS, 0.1, _ptr(ws), wb, _st())
        btail = (m.n_in, m.n_out, m.KV, c_in, c_out, _ptr(m.fwd), _ptr(m.bwd_table), _ptr(w), _ptr(dx), c_in, _ptr(dw), None, _ptr(ws), bb,
                 _st())
        if new:
            L.check(lib.csn_sparse_conv_stats_fwd_t16(_ptr(x), 1, c_in, *tail), "stats t16")
            L.check(lib.csn_sparse_conv_bwd_t16(_ptr(dy), c_out, _ptr(x), 1, c_in, *btail), "bwd t16")
        else:
            L.check(lib.csn_sparse_conv_stats_fwd_f32(_ptr(x), c_in, *tail), "stats f32")
            L.check(lib.csn_sparse_conv_bwd_f32(_ptr(dy), c_out, _ptr(x), c_in, *btail), "bwd f32")
        outs.append((z, mean, invstd, rm, rv, dx, dw))
    return outs


def _assert_conv_equal(L, m, c_in, c_out, seed, what):
    ref, new = _conv_both(L, m, c_in, c_out, seed)
    for q, a, b in zip(("z", "mean", "invstd", "running_mean", "running_var", "dx", "dw"), ref, new):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (what, q, (a - b).abs().max().item())


@pytest.mark.parametrize("c_in,c_out", WIDTHS)
def test_conv_stats_and_weight_gradient_at_tile_edges(L, c_in, c_out):
    for n in SIZES:
        _assert_conv_equal(L, _kmap("s1", n), c_in, c_out, n + c_out, ("s1", n))
    _assert_conv_equal(L, _kmap("s1", "clusters"), c_in, c_out, 5 + c_out, ("s1", "clusters"))


@pytest.mark.parametrize("kind", ["s2", "tr"])
def test_strided_maps(L, kind):
    for c_in, c_out in WIDTHS:
        for n in STRIDED + ["clusters"]:
            m = _kmap(kind, n)
            if m.n_out >= 2:
                _assert_conv_equal(L, m, c_in, c_out, 7 + c_in, (kind, n, c_in, c_out))


def test_every_column_block_count(L):
    lib = L.lib()
    try:
        for c_in, c_out in [(64, 128), (256, 256)]:
            for nb in (1, 2, 3, 4):
                assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) >= 0
                for n in (129, 257):
                    _assert_conv_equal(L, _kmap("s1", n), c_in, c_out, nb + n, ("nb", nb, n, c_out))
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)


def test_flag_zero_is_the_fp32_entry_point_and_two_calls_agree(L):
    lib, m = L.lib(), _kmap("s1", 129)
    a = _conv_both(L, m, 64, 64, 3)
    b = _conv_both(L, m, 64, 64, 3)
    assert all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(m.n_in, 64, generator=g).cuda().bfloat16().float()
    w = (torch.randn(m.KV, 64, 64, generator=g) / (m.KV * 64) ** 0.5).cuda()
    z, mean, invstd = torch.empty(m.n_out, 64, device="cuda"), torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    wb = lib.csn_sparse_conv_stats_workspace_bytes(m.n_out, 64)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    L.check(lib.csn_sparse_conv_stats_fwd_t16(_ptr(x), 0, 64, m.n_in, _ptr(m.fwd), m.n_out, m.KV, 64, 64, _ptr(w), _ptr(z), 64, _ptr(mean),
                                              _ptr(invstd), None, None, H.EPS, 0.1, _ptr(ws), wb, _st()))
    assert torch.equal(z, a[0][0]) and torch.equal(mean, a[0][1]) and torch.equal(invstd, a[0][2])


# ------------------------------------------------------------------------------------------------------
# (28b), (28c) BatchNorm apply + sum + residual + ReLU
# ------------------------------------------------------------------------------------------------------
def _terms(case, M):
    from csn_amd import _lib
    t, keep = _lib.BnTerms(), []
    for m in range(M):
        c = case["terms"][m]
        d = {q: c[q].cuda().contiguous() for q in ("z", "mean", "invstd", "gamma", "beta")}
        keep.append(d)
        t.z[m], t.ld_z[m], t.mean[m], t.scale[m] = _ptr(d["z"]), d["z"].shape[1], _ptr(d["mean"]), _ptr(d["invstd"])
        t.gamma[m], t.beta[m] = _ptr(d["gamma"]), _ptr(d["beta"])
    return t, keep


def _bn_both(L, case, M, n, C, res, relu, y16):
    """Forward and backward through the fp32 entry points and through section 28.  The fp32 forward reads the widened residual; the fp32
    backward masks on the widened bf16 y where section 28 stored bf16.  Returns (y32, y, backward outputs of each)."""
    lib = L.lib()
    r16 = case["r"].cuda().bfloat16() if res else None
    dy = case["dy"].cuda()
    t, keep = _terms(case, M)
    y32 = torch.empty(n, C, device="cuda")
    L.check(lib.csn_rows_bn_act_fwd_f32(ctypes.addressof(t), M, n, C, 1, H.EPS, _ptr(None if r16 is None else r16.float()), C, int(relu),
                                        _ptr(y32), C, _st()), "fwd f32")
    y = torch.empty(n, C, device="cuda", dtype=torch.bfloat16 if y16 else torch.float32)
    L.check(lib.csn_rows_bn_act_fwd_t16(ctypes.addressof(t), M, n, C, 1, H.EPS, _ptr(r16), int(res), C, int(relu), _ptr(y), int(y16), C, _st()),
            "fwd t16")
    wb = lib.csn_rows_bn_act_workspace_bytes(n, C, M)
    grads = []
    for new in (False, True):
        ws = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        dr = torch.empty(n, C, device="cuda") if res else None
        out = []
        for m in range(M):
            dz, dg, db = torch.empty(n, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            t.dz[m], t.ld_dz[m], t.dgamma[m], t.dbeta[m] = _ptr(dz), C, _ptr(dg), _ptr(db)
            out += [dz, dg, db]
        if new:
            L.check(lib.csn_rows_bn_act_bwd_t16(_ptr(dy), C, _ptr(y), int(y16), C, ctypes.addressof(t), M, n, C, 1, H.EPS, int(relu), _ptr(dr),
                                                C, _ptr(ws), wb, _st()), "bwd t16")
        else:
            yw = y.float()
            L.check(lib.csn_rows_bn_act_bwd_f32(_ptr(dy), C, _ptr(yw), C, ctypes.addressof(t), M, n, C, 1, H.EPS, int(relu), _ptr(dr), C,
                                                _ptr(ws), wb, _st()), "bwd f32")
        torch.cuda.synchronize()
        grads.append(out + ([dr] if res else []))
    return y32, y, grads


def _assert_bn_equal(L, case, M, n, C, res, relu, y16, what):
    y32, y, (ref, new) = _bn_both(L, case, M, n, C, res, relu, y16)
    assert bool(torch.isfinite(y32).all())
    if y16:
        assert y.dtype == torch.bfloat16 and torch.equal(y.view(torch.int16), y32.bfloat16().view(torch.int16)), (what, "y")
    else:
        assert torch.equal(y, y32), (what, "y")
    for i, (a, b) in enumerate(zip(ref, new)):
        assert torch.equal(a, b), (what, "backward output", i, (a - b).abs().max().item())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_bn_act_forward_and_backward(L, M, n):
    for C in (32, 96, 256):
        case = bn_act_case(M, n, C)
        for res in (False, True):
            for relu in (True, False):
                for y16 in (True, False):
                    if not (res or y16):
                        continue                                            # nothing 16-bit: section 15 itself
                    _assert_bn_equal(L, case, M, n, C, res, relu, y16, (M, n, C, res, relu, y16))


def test_bn_act_on_zeros_signed_zeros_and_ties(L):
    """Unit statistics, so that v = z + r exactly: exact zeros, -0, negative values that round to -0 in bf16 (below half the smallest
    bf16 subnormal), ties to even, the largest finite values."""
    C, n = 32, 65
    picks = torch.tensor([0.0, -0.0, -1e-41, 1e-41, -1e-30, 1e-30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.0e38, -3.0e38,
                          2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, 0.5])
    g = torch.Generator().manual_seed(9)
    z = picks[torch.randint(0, picks.numel(), (n, C), generator=g)]
    case = {"terms": [{"z": z, "mean": torch.zeros(C), "invstd": torch.ones(C), "gamma": torch.ones(C), "beta": torch.zeros(C)}],
            "r": torch.zeros(n, C), "dy": torch.randn(n, C, generator=g)}
    for res in (False, True):
        for relu in (True, False):
            _assert_bn_equal(L, case, 1, n, C, res, relu, True, ("picks", res, relu))
