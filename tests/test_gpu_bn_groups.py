"""GPU parity of BatchNorm over row groups (include/csn_hip.h section 20; csn_amd/csrc/rows_bn_act.hip ``*_groups``;
csn_amd.minkowski_hrnet ``conv_stats_groups`` / ``bn_act_groups`` / ``merge_batches`` / ``GroupedPyramid``; the tuning switch
``grouped_passes``) against the float64 statement tests/bn_groups_ref.py, in math modes 0 and 1.

Bounds: section 15's own (tests/test_gpu_hrnet.py) — the arithmetic is of the same kind.  Outputs within 1e-4 absolute, each gradient
within 1e-4 of its tensor's max, invstd within 1e-4 max(invstd, invstd^2), running statistics within 1e-4.  z of (20a) must be
``torch.equal`` to section 14's on the same map.  One group must reproduce (15a) / (15b) bit for bit.  Whole blocks and backbones on
three merged groups: the grouped pass's error against float64 is at most max(1e-4, twice the error of the separate passes on the
same case in the same mode) — the rule of ``test_backbone_against_float64``.  Eval on a merged pyramid is ``torch.equal`` to the
groups' own eval passes.

``HRNetSimCSN3S``, K = 2, under ``tuning.override(grouped_passes=True)`` against the switch off, by the same rule: float64 is the
backbone group by group, ``fc_layer`` per group and the head's restatement of tests/test_gpu_minkowski_csn.py; each path's gradients
are taken under that path's own traced ReLU masks.  The true gradient of ``head.fc_layer.0.bias`` is zero (a bias ahead of a
training-mode BatchNorm), so it is measured against the sum over absolute values of its terms.

Group layouts (tests/bn_groups_ref.py ``layout``): row counts 5, 27, 33, 63, 129, 3 (+ the rest) put a boundary inside a 32-row
tile, on a tile edge, inside a 64-row chunk, on a 128-row edge, two inside one tile, and end in a partial tile.  Every group keeps 3
rows or more: a two-row training BatchNorm is ill-conditioned by construction (tests/test_gpu_hrnet.py).

Measured on MI355X, maxima over the cases (fp32 / bf16x3; every test prints its own).  (20a): z 2.1e-6 / 9.8e-6 from float64 (bit-equal
to section 14), mean 3.8e-7 / 2.8e-6, invstd 4.7e-7 / 3.0e-6, running statistics 1.1e-7 / 3.7e-7.  (20b): y 2.9e-6, gradients 2.2e-5 (no
matrix product: the modes agree).  Block on three groups, grouped | separate: y 2.4e-6 / 6.2e-5 | the same, gradients 3.8e-7 / 1.0e-5 | the
same.  Backbone on three groups: 2S y 2.1e-5 / 5.8e-4 | 2.3e-5 / 7.1e-4, gradients 2.4e-6 / 7.0e-5 | 2.5e-6 / 6.2e-5; 3S y 1.7e-5 / 5.9e-4 |
2.0e-5 / 7.4e-4, gradients 4.0e-6 / 7.1e-5 | 3.4e-6 / 1.0e-4; running statistics <= 1.7e-7 / 7.3e-7 | 2.1e-7 / 1.0e-6.  HRNetSimCSN3S, K = 2:
logits 1.8e-6 / 5.2e-5 | 2.3e-6 / 5.1e-5, worst gradient 1.1e-5 / 6.3e-5 | 8.0e-6 / 6.0e-5; grouped against separate logits 1.8e-6 / 1.4e-5."""
import ctypes
import functools

import pytest
import torch

from tests import bn_groups_ref as G
from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
# (mode, set, c_in, c_out, k): 32 -> 32, 64 -> 128 at stride 2, 256 -> 256, the transposed form, the kernel-5 stem
CONVS = [("s1", 260, 32, 32, 3), ("s2", 1031, 64, 128, 3), ("s1", 260, 256, 256, 3), ("tr", 1031, 128, 64, 3), ("s1", 260, 32, 32, 5)]
NETS = {"2S": (2, 4), "3S": (3, 2)}
GROUP_SETS = (31, 33, 129)


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(autouse=True, params=[0, 1], ids=["fp32", "bf16x3"])
def math_mode(request, L):
    L.check(L.lib().csn_set_math_mode(request.param))
    yield request.param
    L.lib().csn_set_math_mode(1)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------
# (20a)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(mode, n, c_in, c_out, k):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = R.random_set(n)
    if mode == "s1":
        g, m = R.geometry("s1", pts, k=k)[0], build_kernel_map(torch.tensor(pts), kernel_size=k)
    else:
        down = build_kernel_map(torch.tensor(pts), kernel_size=3, stride=2)
        if mode == "s2":
            g, m = R.geometry("s2", pts)[0], down
        else:
            g, m = R.geometry("tr", R.down_coords([tuple(c) for c in pts], 1), fine=pts)[0], down.transpose()
    t = R.tensors(n + c_in + 3 * c_out + k, g.n_in, g.n_out, g.KV, c_in, c_out)
    z = R.fwd(g, t["x"], t["w"])
    gen = torch.Generator().manual_seed(c_out)
    rm, rv = 0.1 * torch.randn(c_out, generator=gen), 1 + 0.1 * torch.randn(c_out, generator=gen).abs()
    off = G.layout(g.n_out)
    return g, m, t, z, rm, rv, off, G.stats_groups(z, off, H.EPS, 0.1, rm, rv)


def _stats_groups_gpu(L, case, off, pad=0, running=True):
    g, m, t, _, rm, rv, _, _ = case
    lib = L.lib()
    m = m.to("cuda")
    KV, c_in, c_out = t["w"].shape
    ng = len(off) - 1
    x, w = t["x"].cuda().contiguous(), t["w"].cuda().contiguous()
    zbuf = torch.full((g.n_out, c_out + pad), CANARY, device="cuda")
    mean, invstd = torch.full((ng, c_out), CANARY, device="cuda"), torch.full((ng, c_out), CANARY, device="cuda")
    rm_d, rv_d = (rm.cuda(), rv.cuda()) if running else (None, None)
    wb = lib.csn_sparse_conv_stats_groups_workspace_bytes(g.n_out, c_out, ng)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    grp = _i32(off)
    L.check(lib.csn_sparse_conv_stats_groups_fwd_f32(_ptr(x), c_in, g.n_in, _ptr(m.fwd), g.n_out, KV, c_in, c_out, _ptr(w), _ptr(zbuf),
                                                     c_out + pad, _ptr(mean), _ptr(invstd), _ptr(rm_d), _ptr(rv_d), H.EPS, 0.1, _ptr(grp), ng,
                                                     _ptr(ws), wb, _st()), "stats groups fwd")
    return zbuf, mean, invstd, rm_d, rv_d


def _plain_conv(L, case):
    g, m, t, *_ = case
    m = m.to("cuda")
    KV, c_in, c_out = t["w"].shape
    x, w = t["x"].cuda().contiguous(), t["w"].cuda().contiguous()
    y0 = torch.full((g.n_out, c_out), CANARY, device="cuda")
    L.check(L.lib().csn_sparse_conv_fwd_f32(_ptr(x), c_in, g.n_in, _ptr(m.fwd), g.n_out, KV, c_in, c_out, _ptr(w), None, _ptr(y0), c_out,
                                            _st()), "fwd")
    return y0


def _check_stats(L, case, pad=0):
    g, _, t, z64, _, _, off, ref = case
    c_out = t["w"].shape[2]
    zbuf, mean, invstd, rm_d, rv_d = _stats_groups_gpu(L, case, off, pad)
    y0 = _plain_conv(L, case)
    assert torch.equal(zbuf[:, :c_out], y0), "z differs from csn_sparse_conv_fwd_f32"
    assert bool((zbuf[:, c_out:] == CANARY).all())
    e = {"z": (y0.cpu().double() - z64).abs().max().item(),
         "mean": (mean.cpu().double() - ref["mean"]).abs().max().item(),
         "invstd": ((invstd.cpu().double() - ref["invstd"]).abs() / torch.maximum(ref["invstd"], ref["invstd"] ** 2)).max().item(),
         "rmean": (rm_d.cpu().double() - ref["running_mean"]).abs().max().item(),
         "rvar": (rv_d.cpu().double() - ref["running_var"]).abs().max().item()}
    assert all(v < 1e-4 for v in e.values()), e
    return e


@pytest.mark.parametrize("conv", CONVS, ids=lambda c: f"{c[0]}-{c[2]}-{c[3]}-k{c[4]}")
def test_conv_stats_groups_forward(L, math_mode, conv):
    case = _conv_case(*conv)
    off = case[6]
    assert len(off) - 1 in (6, 7) and min(b - a for a, b in zip(off, off[1:])) >= 3
    e = _check_stats(L, case, pad=8 if conv[2] == 64 else 0)
    print(f"[groups] conv_stats_groups {conv} {len(off) - 1} groups of {off[-1]} rows mode {math_mode}: " + " ".join(f"{q} {v:.1e}" for q, v in e.items()))


def test_conv_stats_groups_pinned_column_blocks_null_running_and_determinism(L, math_mode):
    lib = L.lib()
    case = _conv_case("s1", 260, 256, 256, 3)
    try:
        assert lib.csn_dev_set(L.DEV_SCONV_NB, 3) >= 0
        e = _check_stats(L, case)
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    print(f"[groups] conv_stats_groups pinned column blocks mode {math_mode}: " + " ".join(f"{q} {v:.1e}" for q, v in e.items()))
    off, ref = case[6], case[7]
    a = _stats_groups_gpu(L, case, off, running=False)                     # NULL running pointers: not tracked
    b = _stats_groups_gpu(L, case, off, running=False)
    assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))
    assert (a[1].cpu().double() - ref["mean"]).abs().max() < 1e-4
    c, d = _stats_groups_gpu(L, case, off), _stats_groups_gpu(L, case, off)
    assert all(torch.equal(u, v) for u, v in zip(c, d))                    # two calls give the same bits, running statistics too
    assert all(torch.equal(u, v) for u, v in zip(a[:3], c[:3]))


@pytest.mark.parametrize("conv", CONVS, ids=lambda c: f"{c[0]}-{c[2]}-{c[3]}-k{c[4]}")
def test_one_group_is_conv_stats_bit_for_bit(L, conv):
    case = _conv_case(*conv)
    g, m, t, _, rm, rv, _, _ = case
    lib = L.lib()
    m = m.to("cuda")
    KV, c_in, c_out = t["w"].shape
    x, w = t["x"].cuda().contiguous(), t["w"].cuda().contiguous()
    z, mean, invstd = torch.empty(g.n_out, c_out, device="cuda"), torch.empty(c_out, device="cuda"), torch.empty(c_out, device="cuda")
    rm_d, rv_d = rm.cuda(), rv.cuda()
    wb = lib.csn_sparse_conv_stats_workspace_bytes(g.n_out, c_out)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    L.check(lib.csn_sparse_conv_stats_fwd_f32(_ptr(x), c_in, g.n_in, _ptr(m.fwd), g.n_out, KV, c_in, c_out, _ptr(w), _ptr(z), c_out,
                                              _ptr(mean), _ptr(invstd), _ptr(rm_d), _ptr(rv_d), H.EPS, 0.1, _ptr(ws), wb, _st()))
    got = _stats_groups_gpu(L, case, [0, g.n_out])
    for a, b in zip(got, (z, mean[None], invstd[None], rm_d, rv_d)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------
# (20b)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_act_case(M, n, C):
    """float32 CPU tensors of one (20b) case, never modified; the statistics are the float64 ones of every group, rounded."""
    g = torch.Generator().manual_seed(17 * M + 3 * n + C)
    r = lambda *s: torch.randn(*s, generator=g)
    off = G.layout(n)
    terms = []
    for m in range(M):
        s, o = 0.5 + 0.75 * m, 0.4 * m - 0.3
        z = s * r(n, C) + o
        for i, (lo, hi) in enumerate(zip(off, off[1:])):                     # every group a batch of its own scale and offset
            z[lo:hi] = z[lo:hi] * (1 + 0.5 * i) + 0.7 * i
        st = G.stats_groups(z, off)
        terms.append({"z": z, "gamma": 1 + 0.2 * r(C), "beta": 0.3 * r(C), "mean": st["mean"].float(), "invstd": st["invstd"].float()})
    return {"terms": terms, "r": r(n, C), "dy": r(n, C), "off": off}


def _wide(t, wide, fill):
    if not wide:
        return t.cuda().contiguous(), None
    n, C = t.shape
    buf = torch.full((n, C + 20), fill, dtype=torch.float32, device="cuda")
    buf[:, 8:8 + C] = t.cuda()
    return buf[:, 8:8 + C], buf


def _intact(buf, C, fill):
    return buf is None or (bool((buf[:, :8] == fill).all()) and bool((buf[:, 8 + C:] == fill).all()))


def _bn_act_gpu(L, case, M, n, C, res, relu, wide, skip=False, off=None, stats=None, grouped=True):
    """(20b) forward and backward (twice: the same bits); ``grouped=False``: (15b) in training mode on (C,) statistics."""
    lib = L.lib()
    ld = lambda v: v.stride(0)
    off = case["off"] if off is None else off
    ng = len(off) - 1
    grp = _i32(off)
    T = L.BnTerms()
    keep = []
    for m, t in enumerate(case["terms"]):
        z, _ = _wide(t["z"], wide, 1e30)
        mean, invstd = (t["mean"], t["invstd"]) if stats is None else stats[m]
        vec = [mean.cuda().contiguous(), invstd.cuda().contiguous(), t["gamma"].cuda(), t["beta"].cuda()]
        keep += [z] + vec
        T.z[m], T.ld_z[m], T.mean[m], T.scale[m], T.gamma[m], T.beta[m] = _ptr(z), ld(z), _ptr(vec[0]), _ptr(vec[1]), _ptr(vec[2]), _ptr(vec[3])
    r, _ = _wide(case["r"], wide, 1e30) if res else (None, None)
    y, ybuf = _wide(torch.full((n, C), CANARY), wide, CANARY)
    if grouped:
        L.check(lib.csn_rows_bn_act_groups_fwd_f32(ctypes.addressof(T), M, n, C, _ptr(grp), ng, _ptr(r), ld(r) if res else 0, int(relu),
                                                   _ptr(y), ld(y), _st()), "bn_act groups fwd")
    else:
        L.check(lib.csn_rows_bn_act_fwd_f32(ctypes.addressof(T), M, n, C, 1, H.EPS, _ptr(r), ld(r) if res else 0, int(relu), _ptr(y), ld(y),
                                            _st()), "bn_act fwd")
    assert _intact(ybuf, C, CANARY)
    dy, _ = _wide(case["dy"], wide, 1e30)
    outs = {}
    for rep in range(2):
        dr, drbuf = _wide(torch.full((n, C), CANARY), wide, CANARY)
        o = {"dr": None if (skip or not res) else dr}
        bufs = [drbuf]
        for m in range(M):
            dz, dzbuf = _wide(torch.full((n, C), CANARY), wide, CANARY)
            dg, db = torch.full((C,), CANARY, device="cuda"), torch.full((C,), CANARY, device="cuda")
            o[f"dz{m}"] = None if (skip and m == M - 1) else dz
            o[f"dgamma{m}"] = None if (skip and m == 0) else dg
            o[f"dbeta{m}"] = None if (skip and m == M - 1) else db
            bufs.append(dzbuf)
            T.dz[m], T.ld_dz[m], T.dgamma[m], T.dbeta[m] = _ptr(o[f"dz{m}"]), ld(dz), _ptr(o[f"dgamma{m}"]), _ptr(o[f"dbeta{m}"])
        if grouped:
            wb = lib.csn_rows_bn_act_groups_workspace_bytes(n, C, M, ng)
            ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
            L.check(lib.csn_rows_bn_act_groups_bwd_f32(_ptr(dy), ld(dy), _ptr(y) if relu else None, ld(y), ctypes.addressof(T), M, n, C,
                                                       _ptr(grp), ng, int(relu), _ptr(o["dr"]), ld(dr), _ptr(ws), wb, _st()), "bn_act groups bwd")
        else:
            wb = lib.csn_rows_bn_act_workspace_bytes(n, C, M)
            ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
            L.check(lib.csn_rows_bn_act_bwd_f32(_ptr(dy), ld(dy), _ptr(y) if relu else None, ld(y), ctypes.addressof(T), M, n, C, 1, H.EPS,
                                                int(relu), _ptr(o["dr"]), ld(dr), _ptr(ws), wb, _st()), "bn_act bwd")
        assert all(_intact(b, C, CANARY) for b in bufs)
        outs[rep] = o
    for q, v in outs[0].items():                                           # two calls give the same bits
        assert v is None or torch.equal(v, outs[1][q]), q
    return y, outs[0]


def _bn_act_ref(case, res, relu, y_gpu):
    terms = [{"z": t["z"].double().requires_grad_(True), "gamma": t["gamma"].double().requires_grad_(True),
              "beta": t["beta"].double().requires_grad_(True)} for t in case["terms"]]
    r = case["r"].double().requires_grad_(True) if res else None
    y_true, _ = G.bn_act_groups(terms, case["off"], r, relu)
    y_mask, _ = G.bn_act_groups(terms, case["off"], r, relu, mask=(y_gpu.cpu() > 0) if relu else None)
    leaves = [v for t in terms for v in (t["z"], t["gamma"], t["beta"])] + ([r] if res else [])
    grads = torch.autograd.grad(y_mask, leaves, case["dy"].double())
    ref = {}
    for m in range(len(terms)):
        ref[f"dz{m}"], ref[f"dgamma{m}"], ref[f"dbeta{m}"] = grads[3 * m:3 * m + 3]
    if res:
        ref["dr"] = grads[-1]
    return y_true.detach(), ref


@pytest.mark.parametrize("n", [260, 300])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_bn_act_groups_forward_and_backward(L, math_mode, M, n):
    worst = {"y": 0.0, "grad": 0.0}
    for C in (32, 96, 256):
        case = bn_act_case(M, n, C)
        for res in (False, True):
            for relu in (True, False):
                for wide in (False, True):
                    y, got = _bn_act_gpu(L, case, M, n, C, res, relu, wide)
                    y_ref, ref = _bn_act_ref(case, res, relu, y)
                    ey = (y.cpu().double() - y_ref).abs().max().item()
                    assert ey < 1e-4, (C, res, relu, wide, ey)
                    worst["y"] = max(worst["y"], ey)
                    for q, want in ref.items():
                        eg = (got[q].cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
                        assert eg < 1e-4, (C, res, relu, wide, q, eg)
                        worst["grad"] = max(worst["grad"], eg)
    print(f"[groups] bn_act_groups M={M} rows={n} mode {math_mode}: y {worst['y']:.1e} gradients {worst['grad']:.1e}")


def test_bn_act_groups_skips_null_outputs(L):
    case = bn_act_case(3, 260, 96)
    _, full = _bn_act_gpu(L, case, 3, 260, 96, True, True, True)
    _, part = _bn_act_gpu(L, case, 3, 260, 96, True, True, True, skip=True)
    assert part["dr"] is None and part["dz2"] is None and part["dgamma0"] is None and part["dbeta2"] is None
    for q, v in part.items():
        assert v is None or torch.equal(v, full[q]), q


@pytest.mark.parametrize("n", [260, 1031])
def test_one_group_is_bn_act_bit_for_bit(L, n):
    for M, C in ((1, 32), (2, 96), (3, 256)):
        g = torch.Generator().manual_seed(n + C)
        r = lambda *s: torch.randn(*s, generator=g)
        terms = []
        for m in range(M):
            z = (0.5 + m) * r(n, C) - 0.2
            st = H.stats(z)
            terms.append({"z": z, "gamma": 1 + 0.2 * r(C), "beta": 0.3 * r(C), "mean": st["mean"].float(), "invstd": st["invstd"].float()})
        case = {"terms": terms, "r": r(n, C), "dy": r(n, C), "off": [0, n]}
        for res, relu, wide in ((True, True, False), (False, False, True), (True, True, True)):
            y0, o0 = _bn_act_gpu(L, case, M, n, C, res, relu, wide, grouped=False)
            y1, o1 = _bn_act_gpu(L, case, M, n, C, res, relu, wide, stats=[(t["mean"][None], t["invstd"][None]) for t in terms])
            assert torch.equal(y0, y1)
            for q, v in o0.items():
                assert (v is None and o1[q] is None) or torch.equal(v, o1[q]), (M, C, q)


def test_python_nodes_with_one_group_are_conv_stats_and_bn_act(L):
    from csn_amd import bn_act, bn_act_groups, conv_stats, conv_stats_groups
    g, m, t, *_ = _conv_case("s1", 260, 32, 32, 3)
    m = m.to("cuda")
    outs = []
    for grouped in (False, True):
        x, w = t["x"].cuda().requires_grad_(True), t["w"].cuda().requires_grad_(True)
        gamma, beta = (1 + 0.1 * torch.arange(32.0)).cuda().requires_grad_(True), torch.linspace(-1, 1, 32).cuda().requires_grad_(True)
        rm, rv = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda")
        if grouped:
            off = _i32([0, g.n_out])
            z, mean, invstd = conv_stats_groups(x, w, m, off, rm, rv, 1e-5, 0.1)
            assert mean.shape == (1, 32) and invstd.shape == (1, 32)
            y = bn_act_groups([(z, mean, invstd, gamma, beta)], off, residual=x, relu=True)
        else:
            z, mean, invstd = conv_stats(x, w, m, rm, rv, 1e-5, 0.1)
            y = bn_act([(z, mean, invstd, gamma, beta)], residual=x, relu=True)
        y.backward(t["dy"].cuda())
        outs.append([y.detach(), mean.reshape(-1), invstd.reshape(-1), rm, rv, x.grad, w.grad, gamma.grad, beta.grad])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # needs_input_grad is honoured: no gradient asked of the map or the vectors, none computed
    z = outs[0][0].clone().requires_grad_(False)
    v = torch.ones(1, 32, device="cuda")
    gam = torch.ones(32, device="cuda", requires_grad=True)
    y = bn_act_groups([(z, 0 * v, v, gam, torch.zeros(32, device="cuda"))], _i32([0, z.shape[0]]))
    y.sum().backward()
    assert gam.grad is not None and z.grad is None


# ------------------------------------------------------------------------------------------------------
# merged batches: the block and the backbones on three groups
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sets():
    return [G.sorted_set(n) for n in GROUP_SETS]


@functools.lru_cache(maxsize=None)
def _merged(n_levels, device="cuda"):
    from csn_amd import merge_batches
    return merge_batches([(torch.tensor(s), None) for s in _sets()], n_levels).to(device)


def test_block_on_three_groups_against_float64(L, math_mode):
    from csn_amd import HRBasicBlock, build_kernel_map
    sets = _sets()
    gp = _merged(1)
    off = gp.group_rows_host[0]
    _, p, _, _ = R.block_case()
    gen = torch.Generator().manual_seed(12)
    x, dy = torch.randn(off[-1], 64, generator=gen), torch.randn(off[-1], 64, generator=gen)
    geos = [R.geometry("s1", s)[0] for s in sets]

    def reference(masks):
        p64 = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p.items()}
        x64 = x.double().requires_grad_(True)
        ys = [R.block(geos[i], x64[a:b], p64, True, masks=None if masks is None else [m[a:b] for m in masks])[0]
              for i, (a, b) in enumerate(zip(off, off[1:]))]
        names = [k for k, v in p64.items() if v.requires_grad]
        grads = torch.autograd.grad(torch.cat(ys), [x64] + [p64[k] for k in names], dy.double())
        return torch.cat(ys).detach(), dict(zip(["x"] + names, grads))

    def errors(y, grads, masks):
        y_true, _ = reference(None)
        _, want = reference(masks)
        return {"y": (y.cpu().double() - y_true).abs().max().item(),
                "grad": max((grads[k].cpu().double() - w).abs().max().item() / w.abs().max().item() for k, w in want.items())}

    # separate passes: the block on every group's own map, gradients accumulated
    sep = HRBasicBlock(64, 64).cuda().train()
    sep.load_state_dict(p, strict=False)
    xs = x.cuda().requires_grad_(True)
    ys, m1, m2 = [], [], []
    for i, (a, b) in enumerate(zip(off, off[1:])):
        trace = {}
        ys.append(sep(xs[a:b], build_kernel_map(torch.tensor(sets[i])).to("cuda"), trace, ""))
        m1.append(trace["norm1"].cpu() > 0)
        m2.append(trace["norm2"].cpu() > 0)
    torch.cat(ys).backward(dy.cuda())
    base = errors(torch.cat(ys).detach(), {"x": xs.grad, **{k: v.grad for k, v in sep.named_parameters()}}, (torch.cat(m1), torch.cat(m2)))
    # the grouped pass
    blk = HRBasicBlock(64, 64).cuda().train()
    blk.load_state_dict(p, strict=False)
    xg = x.cuda().requires_grad_(True)
    trace = {}
    y = blk(xg, gp.s1[0], trace, "", gp.group_rows[0])
    y.backward(dy.cuda())
    got = errors(y.detach(), {"x": xg.grad, **{k: v.grad for k, v in blk.named_parameters()}},
                 (trace["norm1"].cpu() > 0, trace["norm2"].cpu() > 0))
    print(f"[groups] block on 3 groups mode {math_mode}: grouped y {got['y']:.1e} gradients {got['grad']:.1e} | "
          f"separate y {base['y']:.1e} gradients {base['grad']:.1e}")
    for q in ("y", "grad"):
        assert got[q] <= max(1e-4, 2 * base[q]), (q, got[q], base[q])
    assert int(blk.norm1.num_batches_tracked) == 3 and int(blk.norm2.num_batches_tracked) == 3
    z1 = torch.cat([R.fwd(geos[i], x[a:b], p["conv1.kernel"]) for i, (a, b) in enumerate(zip(off, off[1:]))])
    s = G.stats_groups(z1, off, 1e-5, 0.02, p["norm1.running_mean"], p["norm1.running_var"])
    assert (blk.norm1.running_mean.cpu().double() - s["running_mean"]).abs().max() < 1e-4
    assert (blk.norm1.running_var.cpu().double() - s["running_var"]).abs().max() < 1e-4


@functools.lru_cache(maxsize=None)
def _backbone_inputs(net):
    S, ff = NETS[net]
    sets = _sets()
    g = torch.Generator().manual_seed(77 + S)
    feats = [torch.randn(len(s), 3, generator=g) for s in sets]
    dys = [torch.randn(len(s), 32 + 32 * ff * (2 ** S - 1), generator=g) for s in sets]
    return [H.Pyramid(s, S) for s in sets], feats, dys


@functools.lru_cache(maxsize=None)
def _backbone_reference(net, training):
    S, ff = NETS[net]
    pyrs, feats, _ = _backbone_inputs(net)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in H.params(S, ff).items()}
    with torch.no_grad():
        rows, _, new = G.backbone_groups(pyrs, [f.double() for f in feats], p, S, training)
    return rows, new


def _masked_gradients(net, masks):
    S, ff = NETS[net]
    pyrs, feats, dys = _backbone_inputs(net)
    p = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in H.params(S, ff).items()}
    f64 = [f.double().requires_grad_(True) for f in feats]
    rows, _, _ = G.backbone_groups(pyrs, f64, p, S, True, masks=masks)
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    grads = torch.autograd.grad(rows, f64 + [p[k] for k in names], [d.double() for d in dys])
    return dict(zip([f"feats{i}" for i in range(len(f64))] + names, grads))


def _backbone_errors(net, rows, got, masks, sd):
    ref_rows, new = _backbone_reference(net, True)
    want = _masked_gradients(net, masks)
    assert sorted(got) == sorted(want)
    e = {"y": max((r.detach().cpu().double() - w).abs().max().item() for r, w in zip(rows, ref_rows)),
         "grad": max((got[k].cpu().double() - w).abs().max().item() / max(w.abs().max().item(), 1e-300) for k, w in want.items()),
         "running": 0.0}
    for name, (rm, rv) in new.items():
        e["running"] = max(e["running"], (sd[name + ".running_mean"].cpu().double() - rm).abs().max().item(),
                           (sd[name + ".running_var"].cpu().double() - rv).abs().max().item())
        assert int(sd[name + ".num_batches_tracked"]) == len(GROUP_SETS), name
    return e


def _run_separate(net):
    from csn_amd import HRNetBackbone, build_pyramid
    S, ff = NETS[net]
    _, feats, dys = _backbone_inputs(net)
    bb = HRNetBackbone(3, S, ff).cuda().train()
    bb.load_state_dict(H.params(S, ff))
    rows, masks, xs = [], [], []
    for s, f, d in zip(_sets(), feats, dys):
        x = f.cuda().requires_grad_(True)
        trace = {}
        y = bb(x, build_pyramid(torch.tensor(s), S).to("cuda"), trace)
        y.backward(d.cuda())
        rows.append(y)
        xs.append(x)
        masks.append({k: v.cpu() > 0 for k, v in trace.items()})
    got = {**{f"feats{i}": x.grad for i, x in enumerate(xs)}, **{k: v.grad for k, v in bb.named_parameters()}}
    return _backbone_errors(net, rows, got, masks, bb.state_dict())


def _run_grouped(net, keep=None):
    from csn_amd import HRNetBackbone
    S, ff = NETS[net]
    _, feats, dys = _backbone_inputs(net)
    gp = _merged(S)
    bb = HRNetBackbone(3, S, ff).cuda().train()
    bb.load_state_dict(H.params(S, ff))
    x = torch.cat(feats).cuda().requires_grad_(True)
    trace = {}
    y = bb(x, gp, trace)
    y.backward(torch.cat(dys).cuda())
    if keep is not None:
        keep += [y.detach(), x.grad] + [v.grad for v in bb.parameters()] + [v for k, v in bb.state_dict().items() if "running" in k]
    level = {gp.group_rows_host[l][-1]: l for l in range(S)}
    assert len(level) == S                                                  # (the levels' row counts tell them apart)
    masks = [{} for _ in GROUP_SETS]
    for k, v in trace.items():
        off = gp.group_rows_host[level[v.shape[0]]]
        for i, (a, b) in enumerate(zip(off, off[1:])):
            masks[i][k] = v[a:b].cpu() > 0
    off = gp.group_rows_host[0]
    got = {**{f"feats{i}": x.grad[a:b] for i, (a, b) in enumerate(zip(off, off[1:]))}, **{k: v.grad for k, v in bb.named_parameters()}}
    return _backbone_errors(net, [y[a:b] for a, b in zip(off, off[1:])], got, masks, bb.state_dict())


@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_on_three_groups_against_float64(L, math_mode, net):
    base = _run_separate(net)
    got = _run_grouped(net)
    print(f"[groups] backbone {net} on 3 groups mode {math_mode}: grouped y {got['y']:.1e} gradients {got['grad']:.1e} running "
          f"{got['running']:.1e} | separate y {base['y']:.1e} gradients {base['grad']:.1e} running {base['running']:.1e}")
    for q in ("y", "grad", "running"):
        assert got[q] <= max(1e-4, 2 * base[q]), (q, got[q], base[q])


def test_two_grouped_calls_give_the_same_bits(L, math_mode):
    a, b = [], []
    _run_grouped("3S", a)
    _run_grouped("3S", b)
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_unfused_training_on_groups_raises(L):
    from csn_amd import HRNetBackbone
    bb = HRNetBackbone(3, 2, 4, fused=False).cuda().train()
    with pytest.raises(ValueError, match="fused"):
        bb(torch.zeros(_merged(2).coords[0].shape[0], 3, device="cuda"), _merged(2))


@pytest.mark.parametrize("epilogue", [False, True], ids=["two-launch", "eval_epilogue"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_eval_on_a_merged_pyramid_equals_the_groups_own_eval(L, math_mode, net, epilogue):
    from csn_amd import HRNetBackbone, build_pyramid, tuning
    S, ff = NETS[net]
    _, feats, _ = _backbone_inputs(net)
    gp = _merged(S)
    bb = HRNetBackbone(3, S, ff).cuda().eval()
    bb.load_state_dict(H.params(S, ff))
    with torch.no_grad(), tuning.override(eval_epilogue=epilogue):
        y = bb(torch.cat(feats).cuda(), gp)
        own = [bb(f.cuda(), build_pyramid(torch.tensor(s), S).to("cuda")) for s, f in zip(_sets(), feats)]
    assert torch.equal(y, torch.cat(own))
    assert all(int(v) == 0 for k, v in bb.state_dict().items() if k.endswith("num_batches_tracked"))


# ------------------------------------------------------------------------------------------------------
# HRNetSimCSN3S under the switch
# ------------------------------------------------------------------------------------------------------
def _count_calls(L, fn):
    calls = {}

    def hook(name, phase):
        if phase == "begin":
            calls[name] = calls.get(name, 0) + 1
    L.set_call_hook(hook)
    try:
        out = fn()
    finally:
        L.set_call_hook(None)
    return out, calls


def _batch(seed):
    pts = G.sorted_set(65, seed=seed)
    g = torch.Generator().manual_seed(50 + seed)
    return torch.tensor(pts), torch.randn(len(pts), 3, generator=g).cuda()


def _shape_offsets(coords):
    from csn_amd.minkowski_csn import offsets_from_batch_index
    return [int(v) for v in offsets_from_batch_index(coords[:, 0]).tolist()]


def _model64(sd, batches, masks=None, fc_masks=None):
    """``HRNetSimCSN3S`` (K = len(batches) - 1, training, no dropout) in float64 on the state dict ``sd``: the backbone group by
    group (tests/bn_groups_ref.py), ``fc_layer`` per group (Linear + training BatchNorm + ReLU), the head of
    tests/test_gpu_minkowski_csn.py.  ``masks`` / ``fc_masks``: per group the 0/1 masks that stand in for the ReLUs.  Returns the
    logits, the float64 parameters (leaves) and the pre-BatchNorm rows of ``fc_layer`` per group (their gradients are retained)."""
    import torch.nn.functional as F
    from tests.test_gpu_minkowski_csn import ref_head
    p = {k: (v.detach().cpu().double().requires_grad_("running" not in k) if v.is_floating_point() else v.cpu()) for k, v in sd.items()}
    pb = {k[len("backbone."):]: v for k, v in p.items() if k.startswith("backbone.")}
    pyrs = [H.Pyramid(c.tolist(), 3) for c, _ in batches]
    rows, _, _ = G.backbone_groups(pyrs, [f.cpu().double() for _, f in batches], pb, 3, True, masks)
    W, b, gam, bet = (p[f"head.fc_layer.{q}"] for q in ("0.weight", "0.bias", "1.weight", "1.bias"))
    lins, shapes = [], []
    for g, r in enumerate(rows):
        lin = r @ W.t() + b
        if lin.requires_grad:
            lin.retain_grad()
        lins.append(lin)
        a = F.batch_norm(lin, None, None, gam, bet, True, 0.0, 1e-5)
        y = a.clamp_min(0) if fc_masks is None else a * fc_masks[g].double()
        off = _shape_offsets(batches[g][0])
        shapes.append([y[lo:hi] for lo, hi in zip(off, off[1:])])
    ph = {k[len("head."):]: v for k, v in p.items() if k.startswith("head.") and ".fc_layer." not in k}
    return ref_head(shapes[0], shapes[1:], ph, 2, 64), p, lins


def _simcsn_step(L, grouped):
    """One training step of HRNetSimCSN3S, K = 2, with the switch on or off: the logits, every parameter's gradient, the traced ReLU
    masks per group (the backbone's and fc_layer's), the C calls, the stem's statistics."""
    from csn_amd import GroupedPyramid, HRNetSimCSN3S, tuning
    torch.manual_seed(4)
    model = HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=2, dropout=0.0).cuda().train()
    model.head.MHA.dropout.p = model.head.MHA.attention.dropout.p = 0.0    # (the attention's own dropout keeps the reference's 0.1)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    batches = [_batch(0), _batch(1), _batch(2)]
    traces, fc_masks = [], []
    inner = model.backbone.forward

    def traced(feats, pyramid, trace=None):
        traces.append(({}, pyramid))
        return inner(feats, pyramid, traces[-1][0])
    model.backbone.forward = traced
    hook = model.head.fc_layer.register_forward_hook(lambda mod, args, out: fc_masks.append(out.detach().cpu() > 0))
    with tuning.override(grouped_passes=grouped):
        logits, calls = _count_calls(L, lambda: model(batches[0], batches[1:]))
        logits.square().mean().backward()
    hook.remove()
    assert len(fc_masks) == 3
    if grouped:
        assert len(traces) == 1 and isinstance(traces[0][1], GroupedPyramid)
        trace, gp = traces[0]
        level = {gp.group_rows_host[l][-1]: l for l in range(3)}
        assert len(level) == 3
        masks = [{} for _ in batches]
        for k, v in trace.items():
            off = gp.group_rows_host[level[v.shape[0]]]
            for i, (a, b) in enumerate(zip(off, off[1:])):
                masks[i][k] = v[a:b].cpu() > 0
    else:
        assert len(traces) == 3
        masks = [{k: v.cpu() > 0 for k, v in t.items()} for t, _ in traces]
    grads = {k: v.grad.cpu().double() for k, v in model.named_parameters()}
    stem = model.backbone.bn0s1
    return {"sd": sd, "batches": batches, "logits": logits.detach().cpu().double(), "grads": grads, "masks": masks, "fc_masks": fc_masks,
            "calls": calls, "stem": (stem.running_mean.clone(), stem.running_var.clone(), int(stem.num_batches_tracked))}


def _simcsn_errors(run, logits_true):
    """Errors of one step against float64: the logits absolute (true ReLUs), every parameter gradient relative to its tensor's max
    under the step's own masks.  ``head.fc_layer.0.bias`` sits ahead of a training-mode BatchNorm, which projects it out: its true
    gradient is zero, so it is measured against the same sum over absolute values of its terms (the project's convention for
    gradients that cancel)."""
    logits, p, lins = _model64(run["sd"], run["batches"], run["masks"], run["fc_masks"])
    logits.square().mean().backward()
    e = {"logits": (run["logits"] - logits_true).abs().max().item()}
    for k, got in run["grads"].items():
        want = p[k].grad
        scale = want.abs().max().item()
        if k == "head.fc_layer.0.bias":
            scale = sum(l.grad.abs().sum(0) for l in lins).max().item()
        e[k] = (got - want).abs().max().item() / max(scale, 1e-300)
    return e


def test_simcsn3s_switch_against_float64_and_the_separate_passes(L, math_mode):
    sep, grp = _simcsn_step(L, False), _simcsn_step(L, True)
    with torch.no_grad():
        logits_true = _model64(sep["sd"], sep["batches"])[0]
    e_sep, e_grp = _simcsn_errors(sep, logits_true), _simcsn_errors(grp, logits_true)
    wg, ws = max((k for k in e_grp if k != "logits"), key=e_grp.get), max((k for k in e_sep if k != "logits"), key=e_sep.get)
    print(f"[groups] HRNetSimCSN3S K=2 mode {math_mode}: grouped logits {e_grp['logits']:.1e} worst gradient {e_grp[wg]:.1e} ({wg}) | "
          f"separate logits {e_sep['logits']:.1e} worst gradient {e_sep[ws]:.1e} ({ws}); grouped - separate logits "
          f"{(grp['logits'] - sep['logits']).abs().max().item():.1e}")
    for k in e_sep:
        assert e_grp[k] <= max(1e-4, 2 * e_sep[k]), (k, e_grp[k], e_sep[k])
    assert grp["stem"][2] == sep["stem"][2] == 3
    assert (grp["stem"][0] - sep["stem"][0]).abs().max() < 1e-4 and (grp["stem"][1] - sep["stem"][1]).abs().max() < 1e-4
    cs, cg = sep["calls"], grp["calls"]
    assert cs.get("csn_sparse_conv_stats_fwd_f32") == 3 * 47 and "csn_sparse_conv_stats_groups_fwd_f32" not in cs
    assert cg.get("csn_sparse_conv_stats_groups_fwd_f32") == 47 and "csn_sparse_conv_stats_fwd_f32" not in cg
    assert cg.get("csn_rows_fc_fwd_f32") == cs.get("csn_rows_fc_fwd_f32") == 3      # fc_layer: once per group, as before


def test_simcsn3s_takes_a_grouped_pyramid_as_queries(L, math_mode):
    from csn_amd import HRNetSimCSN3S, merge_batches, tuning
    torch.manual_seed(4)
    model = HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=2, dropout=0.0).cuda().eval()
    q, keys = _batch(0), [_batch(1), _batch(2)]
    gp = merge_batches([q] + keys, 3, n_shapes=[2, 2, 2])
    feats = torch.cat([f for _, f in [q] + keys])
    with torch.no_grad():
        a = model((gp, feats))
        with tuning.override(grouped_passes=True):
            b = model(q, keys)
        c = model(q, keys)
    assert a.shape == (q[0].shape[0], 6) and torch.equal(a, b) and torch.equal(a, c)      # eval: the same bits as the separate passes
    with pytest.raises(ValueError, match="keys=None"):
        model((gp, feats), keys)


def test_merged_point_batch_is_the_separate_batches_with_running_item_numbers(L):
    """``PointCollection.merged_batch``: the queries' batch and the K neighbour batches as one collation; its voxel set under
    ``group_pyramid`` has the groups of ``merge_batches`` on the separate batches' voxel sets."""
    import numpy as np
    from csn_amd import group_pyramid, merge_batches
    from csn_amd.minkowski_points import PointCollection
    rng = np.random.default_rng(3)
    col = PointCollection([rng.standard_normal((40 + 7 * s, 3)).astype(np.float32) for s in range(6)])
    q_idx, nbrs, K = [4, 1], [(4, [0, 2]), (1, [5, 3])], 2
    merged = col.merged_batch(q_idx, nbrs, K, voxel_size=0.25)
    parts = [col.batch(q_idx, None, 0.25)] + col.neighbor_batches(nbrs, K, None, 0.25)
    assert merged.group_shapes == [2, 2, 2] and merged.n_shapes == 6
    want = torch.cat([p.coords + torch.tensor([2.0 * g, 0, 0, 0], device="cuda") for g, p in enumerate(parts)])
    assert torch.equal(merged.coords, want) and torch.equal(merged.feats, torch.cat([p.feats for p in parts]))
    gp = group_pyramid(merged.field().voxel_coords, merged.group_shapes, 2)
    ref = merge_batches([(p.field().voxel_coords, None) for p in parts], 2, n_shapes=[2, 2, 2])
    assert gp.group_rows_host == ref.group_rows_host and gp.row_offsets == ref.row_offsets
    assert all(torch.equal(a, b) for a, b in zip(gp.coords, ref.coords)) and torch.equal(gp.s1[1].fwd, ref.s1[1].fwd)


def test_the_trainers_forward_picks_the_switch_up(L):
    """``csn_amd.minkowski_trainer``'s ``forward_fn`` (what ``train_iter`` and ``evaluate`` call on a collated batch of point fields)
    under ``tuning.grouped_passes``: no flag of its own — the fields' voxel coordinates are merged inside ``HRNetSimCSN.forward``.
    Eval: the same bits as with the switch off.  Training: one grouped call per convolution instead of K + 1 calls, a finite loss
    and a gradient for every parameter."""
    from csn_amd import HRNetSimCSN2S, PointCollection, tuning
    from csn_amd.minkowski_trainer import _collate, _forward
    from csn_amd.train_csn import synthetic_shapes
    pts, labs = synthetic_shapes(4, seed=3)
    col = PointCollection(pts, labs)
    neighbors = {0: (0, [2]), 1: (1, [3])}
    batch, target = _collate(col, col, [0, 1], neighbors, 1, None, 0.05, (0.01, 0.05), "random_subsample")
    torch.manual_seed(11)
    model = HRNetSimCSN2S(3, 9, d_model=64, n_head=2, k_neighbors=1).cuda().eval()
    with torch.no_grad():
        off, _ = _forward(model, batch)
        with tuning.override(grouped_passes=True):
            on, _ = _forward(model, batch)
    assert off.shape == (target.shape[0], 9) and torch.equal(on, off)
    model.train()
    (_, _), calls_off = _count_calls(L, lambda: _forward(model, batch))
    with tuning.override(grouped_passes=True):
        (logits, _), calls_on = _count_calls(L, lambda: _forward(model, batch))
        loss = torch.nn.functional.cross_entropy(logits, target.long().clamp(0, 8))
        loss.backward()
    n_convs = calls_on.get("csn_sparse_conv_stats_groups_fwd_f32")
    assert n_convs and calls_off.get("csn_sparse_conv_stats_fwd_f32") == 2 * n_convs and "csn_sparse_conv_stats_fwd_f32" not in calls_on
    assert bool(torch.isfinite(loss))
    for name, prm in model.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
