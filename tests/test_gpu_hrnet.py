"""GPU parity of the HRNet backbone on voxel rows (csn_amd/minkowski_hrnet.py; csn_amd/csrc/rows_bn_act.hip and the statistics
epilogue of csn_amd/csrc/sparse_conv.hip; include/csn_hip.h section 15) against the float64 restatement tests/hrnet_ref.py, in math
modes 0 and 1.

(15a) on point sets either side of the 32-row wave and 128-row work-group tiles, at every width the backbone uses, the kernel-5
stem, stride 2 and the transposed form, and with the column blocks per wave pinned: z bit-equal to ``csn_sparse_conv_fwd_f32``;
mean, invstd and the running statistics against float64.  (15b) for 1 / 2 / 3 terms x residual x ReLU x training / eval at 2, 63,
65 and 1031 rows (either side of the 64-row chunk) and 32 / 96 / 256 columns, at natural pitches and as column blocks of wider
buffers with canaries; NULL outputs; determinism.  ``HRBasicBlock``, ``HRNetBackbone`` 2S / 3S and ``HRNetSimCSN3S`` through autograd.

Bounds.  Single operations and the block: outputs within 1e-4 absolute, each gradient within 1e-4 of its tensor's max (the project's
contract).  invstd is a derived quantity: an error dz of the map moves it by invstd^2 dz (d invstd = -invstd^3 d var / 2, d var = 2
std dz), so it is held to 1e-4 max(invstd, invstd^2).  A training-mode BatchNorm over TWO rows has a gradient that cancels to zero
(two rows span {1, xhat}: everything is projected out), so dz at 2 rows is measured against the same formula over absolute values
of its terms, as tests/sparse_conv_ref.py does for its cancelling gradients.  Whole networks pass up to 47 normalisations: the test
runs ``fused=False`` (``sparse_conv3d`` + ATen: the arithmetic the project had before) on the same case in the same mode, measures
ITS error against float64, and ``fused=True`` may have at most the larger of 1e-4 and twice that; outputs absolute, gradients
relative to each tensor's max, gradients of both paths taken against float64 under that path's own traced ReLU masks.

Measured on MI355X, maxima over the cases (fp32 / bf16x3; every test prints its own).  (15a): z 7.9e-6 / 1.5e-5 from float64 (bit-equal
to section 14), mean 3.3e-7 / 3.0e-6, invstd 3.5e-7 / 3.1e-6, running statistics 1.0e-7 / 4.1e-7.  (15b): y 1.4e-6, gradients 1.7e-7;
at 2 rows y 1.2e-5, gradients 4.3e-6 (no matrix product: the modes agree).  Block: y 3.2e-6 / 4.6e-5 (training), gradients 4.7e-7 /
8.1e-6, within 1.4e-6 / 7.2e-6 of ``SparseBasicBlock``.  Backbone on 300 voxels, fused | unfused: 2S training y 1.6e-5 / 2.5e-4 |
1.8e-5 / 2.4e-4, gradients 3.3e-6 / 2.6e-5 | 3.3e-6 / 2.9e-5; 3S training y 1.6e-5 / 3.3e-4 | 2.0e-5 / 3.5e-4, gradients 5.3e-6 / 3.1e-5
| 4.0e-6 / 3.0e-5; eval y <= 1.2e-6 / 1.1e-5 | 1.2e-6 / 9.3e-6, gradients <= 2.6e-6 / 1.4e-5 | 3.2e-6 / 1.4e-5; running statistics
<= 1.1e-7 / 3.4e-7 | 1.4e-7 / 3.8e-7.  The set with 2 coarsest rows, training (ill-conditioned by construction: a two-row BatchNorm
divides by half the distance of two nearly equal values, and both paths show it): 2S y 2.7e-3 / 1.4e-2 | 2.9e-3 / 2.4e-2, gradients
2.6e-2 / 1.5e-1 | 3.0e-2 / 1.4e-1; 3S y 1.9e-2 / 2.1e-1 | 3.2e-2 / 1.2e-1, gradients 5.1e-1 / 8.1e-1 | 4.8e-1 / 1.6; in eval the same
set gives y <= 2.0e-6 / 2.1e-5 on both paths.  HRNetSimCSN3S: the stem's running mean after K + 1 batches within 1e-10 / 4e-9."""
import ctypes
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
NETS = {"2S": (2, 4), "3S": (3, 2)}
TWO_ROWS = [[0, 1, 0, 0], [0, 2, 0, 0]]               # neighbours at stride 1; two coarse rows at stride 2
SETS = {"rand31": lambda: R.random_set(31), "rand33": lambda: R.random_set(33), "rand129": lambda: R.random_set(129),
        "rand1031": lambda: R.random_set(1031), "clusters": R.two_clusters, "two": lambda: TWO_ROWS}
# (mode, c_in, c_out, k): the widths of the backbone, the stem (3 colours padded to 32), stride 2 and the transposed form
CONVS = [("s1", 32, 32, 3), ("s1", 64, 64, 3), ("s1", 128, 128, 3), ("s1", 256, 256, 3), ("s1", 32, 32, 5), ("s2", 64, 128, 3),
         ("tr", 128, 64, 3)]
NB_CASES = [(64, 64, 2), (96, 96, 3), (128, 128, 4), (256, 256, 3)]


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


# ------------------------------------------------------------------------------------------------------
# (15a)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(mode, name, c_in, c_out, k):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = SETS[name]()
    if mode == "s1":
        g, m = R.geometry("s1", pts, k=k)[0], build_kernel_map(torch.tensor(pts), kernel_size=k)
    else:
        down = build_kernel_map(torch.tensor(pts), kernel_size=3, stride=2)
        if mode == "s2":
            g, m = R.geometry("s2", pts)[0], down
        else:
            g, m = R.geometry("tr", R.down_coords([tuple(c) for c in pts], 1), fine=pts)[0], down.transpose()
    t = R.tensors(len(name) + c_in + 3 * c_out + k, g.n_in, g.n_out, g.KV, c_in, c_out)
    z = R.fwd(g, t["x"], t["w"])
    gen = torch.Generator().manual_seed(c_out)
    rm, rv = 0.1 * torch.randn(c_out, generator=gen), 1 + 0.1 * torch.randn(c_out, generator=gen).abs()
    return g, m, t, z, rm, rv, H.stats(z, H.EPS, 0.1, rm, rv)


def _run_conv_stats(L, case, pad=0):
    g, m, t, z64, rm, rv, ref = case
    lib = L.lib()
    m = m.to("cuda")
    KV, c_in, c_out = t["w"].shape
    x, w = t["x"].cuda().contiguous(), t["w"].cuda().contiguous()
    zbuf = torch.full((g.n_out, c_out + pad), CANARY, device="cuda")
    y0 = torch.full((g.n_out, c_out), CANARY, device="cuda")
    mean, invstd = torch.full((c_out,), CANARY, device="cuda"), torch.full((c_out,), CANARY, device="cuda")
    rm_d, rv_d = rm.cuda(), rv.cuda()
    wb = lib.csn_sparse_conv_stats_workspace_bytes(g.n_out, c_out)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    L.check(lib.csn_sparse_conv_fwd_f32(_ptr(x), c_in, g.n_in, _ptr(m.fwd), g.n_out, KV, c_in, c_out, _ptr(w), None, _ptr(y0), c_out,
                                        _st()), "fwd")
    L.check(lib.csn_sparse_conv_stats_fwd_f32(_ptr(x), c_in, g.n_in, _ptr(m.fwd), g.n_out, KV, c_in, c_out, _ptr(w), _ptr(zbuf),
                                              c_out + pad, _ptr(mean), _ptr(invstd), _ptr(rm_d), _ptr(rv_d), H.EPS, 0.1, _ptr(ws), wb,
                                              _st()), "stats fwd")
    assert torch.equal(zbuf[:, :c_out], y0), "z differs from csn_sparse_conv_fwd_f32"
    assert bool((zbuf[:, c_out:] == CANARY).all())
    e = {"z": (y0.cpu().double() - z64).abs().max().item(),
         "mean": (mean.cpu().double() - ref["mean"]).abs().max().item(),
         "invstd": ((invstd.cpu().double() - ref["invstd"]).abs() / torch.maximum(ref["invstd"], ref["invstd"] ** 2)).max().item(),
         "rmean": (rm_d.cpu().double() - ref["running_mean"]).abs().max().item(),
         "rvar": (rv_d.cpu().double() - ref["running_var"]).abs().max().item()}
    assert all(v < 1e-4 for v in e.values()), e
    return e, (zbuf, mean, invstd, rm_d, rv_d)


@pytest.mark.parametrize("name", list(SETS))
def test_conv_stats_forward(L, math_mode, name):
    worst = {}
    for i, (mode, c_in, c_out, k) in enumerate(CONVS):
        e, _ = _run_conv_stats(L, _conv_case(mode, name, c_in, c_out, k), pad=8 if i % 2 else 0)
        worst = {q: max(v, worst.get(q, 0.0)) for q, v in e.items()}
    print(f"[hrnet] conv_stats {name} mode {math_mode}: " + " ".join(f"{q} {v:.1e}" for q, v in worst.items()))


def test_conv_stats_with_pinned_column_blocks_and_null_running(L, math_mode):
    lib = L.lib()
    worst = {}
    try:
        for c_in, c_out, nb in NB_CASES:
            assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) >= 0
            e, _ = _run_conv_stats(L, _conv_case("s1", "rand1031", c_in, c_out, 3))
            worst = {q: max(v, worst.get(q, 0.0)) for q, v in e.items()}
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    print(f"[hrnet] conv_stats pinned column blocks mode {math_mode}: " + " ".join(f"{q} {v:.1e}" for q, v in worst.items()))
    # NULL running pointers: not tracked; two calls give the same bits
    g, m, t, _, _, _, ref = _conv_case("s1", "rand129", 64, 64, 3)
    m = m.to("cuda")
    x, w = t["x"].cuda(), t["w"].cuda()
    outs = []
    for _ in range(2):
        z, mean, invstd = (torch.empty(g.n_out, 64, device="cuda"), torch.empty(64, device="cuda"), torch.empty(64, device="cuda"))
        wb = lib.csn_sparse_conv_stats_workspace_bytes(g.n_out, 64)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        L.check(lib.csn_sparse_conv_stats_fwd_f32(_ptr(x), 64, g.n_in, _ptr(m.fwd), g.n_out, 27, 64, 64, _ptr(w), _ptr(z), 64, _ptr(mean),
                                                  _ptr(invstd), None, None, H.EPS, 0.1, _ptr(ws), wb, _st()))
        outs.append((z, mean, invstd))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert (outs[0][1].cpu().double() - ref["mean"]).abs().max() < 1e-4


def test_conv_stats_refuses_a_single_voxel(L):
    from csn_amd import conv_stats
    from csn_amd.minkowski_conv import build_kernel_map
    m = build_kernel_map(torch.tensor(R.single_voxel())).to("cuda")
    x, w = torch.zeros(1, 32, device="cuda"), torch.zeros(27, 32, 32, device="cuda")
    z, v = torch.zeros(1, 32, device="cuda"), torch.zeros(32, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    assert L.lib().csn_sparse_conv_stats_fwd_f32(_ptr(x), 32, 1, _ptr(m.fwd), 1, 27, 32, 32, _ptr(w), _ptr(z), 32, _ptr(v), _ptr(v), None,
                                                 None, 1e-5, 0.02, _ptr(ws), 4096, _st()) == -1
    with pytest.raises(ValueError, match="more than 1 value"):
        conv_stats(x, w, m, None, None, 1e-5, 0.02)


# ------------------------------------------------------------------------------------------------------
# (15b)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_act_case(M, n, C):
    """float32 CPU tensors of one (15b) case, never modified: maps of different scale and offset per term."""
    g = torch.Generator().manual_seed(17 * M + 3 * n + C)
    r = lambda *s: torch.randn(*s, generator=g)
    terms = []
    for m in range(M):
        s, o = 0.5 + 0.75 * m, 0.4 * m - 0.3
        z = s * r(n, C) + o
        st = H.stats(z)
        terms.append({"z": z, "gamma": 1 + 0.2 * r(C), "beta": 0.3 * r(C), "running_mean": o + 0.1 * r(C),
                      "running_var": s * s * (1 + 0.1 * r(C).abs()), "mean": st["mean"].float(), "invstd": st["invstd"].float()})
    return {"terms": terms, "r": r(n, C), "dy": r(n, C)}


def _wide(t, wide, fill):
    """(n, C) CPU tensor -> a device view; ``wide``: columns [8, 8 + C) of an (n, C + 20) buffer filled with ``fill``."""
    if not wide:
        return t.cuda().contiguous(), None
    n, C = t.shape
    buf = torch.full((n, C + 20), fill, dtype=torch.float32, device="cuda")
    buf[:, 8:8 + C] = t.cuda()
    return buf[:, 8:8 + C], buf


def _intact(buf, C, fill):
    return buf is None or (bool((buf[:, :8] == fill).all()) and bool((buf[:, 8 + C:] == fill).all()))


def _bn_act_gpu(L, case, M, n, C, res, relu, training, wide, skip=False):
    lib = L.lib()
    ld = lambda v: v.stride(0)
    T = L.BnTerms()
    keep = []
    for m, t in enumerate(case["terms"]):
        z, _ = _wide(t["z"], wide, 1e30)
        vec = [t[q].cuda() for q in (("mean", "invstd") if training else ("running_mean", "running_var"))] + [t["gamma"].cuda(), t["beta"].cuda()]
        keep += [z] + vec
        T.z[m], T.ld_z[m], T.mean[m], T.scale[m], T.gamma[m], T.beta[m] = _ptr(z), ld(z), _ptr(vec[0]), _ptr(vec[1]), _ptr(vec[2]), _ptr(vec[3])
    r, _ = _wide(case["r"], wide, 1e30) if res else (None, None)
    y, ybuf = _wide(torch.full((n, C), CANARY), wide, CANARY)
    L.check(lib.csn_rows_bn_act_fwd_f32(ctypes.addressof(T), M, n, C, int(training), H.EPS, _ptr(r), ld(r) if res else 0, int(relu),
                                        _ptr(y), ld(y), _st()), "bn_act fwd")
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
        wb = lib.csn_rows_bn_act_workspace_bytes(n, C, M)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        L.check(lib.csn_rows_bn_act_bwd_f32(_ptr(dy), ld(dy), _ptr(y) if relu else None, ld(y), ctypes.addressof(T), M, n, C, int(training),
                                            H.EPS, int(relu), _ptr(o["dr"]), ld(dr), _ptr(ws), wb, _st()), "bn_act bwd")
        assert all(_intact(b, C, CANARY) for b in bufs)
        outs[rep] = o
    for q, v in outs[0].items():                                           # two calls give the same bits
        assert v is None or torch.equal(v, outs[1][q]), q
    return y, outs[0]


def _bn_act_ref(case, res, relu, training, y_gpu):
    terms = []
    for t in case["terms"]:
        terms.append({"z": t["z"].double().requires_grad_(True), "gamma": t["gamma"].double().requires_grad_(True),
                      "beta": t["beta"].double().requires_grad_(True), "running_mean": t["running_mean"].double(),
                      "running_var": t["running_var"].double()})
    r = case["r"].double().requires_grad_(True) if res else None
    y_true, _ = H.bn_act(terms, r, relu, training)
    y_mask, _ = H.bn_act(terms, r, relu, training, mask=(y_gpu.cpu() > 0) if relu else None)
    leaves = [v for t in terms for v in (t["z"], t["gamma"], t["beta"])] + ([r] if res else [])
    grads = torch.autograd.grad(y_mask, leaves, case["dy"].double())
    ref = {}
    for m in range(len(terms)):
        ref[f"dz{m}"], ref[f"dgamma{m}"], ref[f"dbeta{m}"] = grads[3 * m:3 * m + 3]
    if res:
        ref["dr"] = grads[-1]
    # the dz formula over absolute values of its terms: the scale where the true dz cancels (two rows, training)
    scales = {}
    if training:
        g = case["dy"].double().abs() * ((y_gpu.cpu() > 0).double() if relu else 1.0)
        for m, t in enumerate(case["terms"]):
            st = H.stats(t["z"])
            xh = ((t["z"].double() - st["mean"]) * st["invstd"]).abs()
            scales[f"dz{m}"] = ((t["gamma"].double().abs() * st["invstd"]) * (g + g.mean(0) + xh * (g * xh).mean(0))).max().item()
    return y_true.detach(), ref, scales


@pytest.mark.parametrize("n", [2, 63, 65, 1031])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_bn_act_forward_and_backward(L, math_mode, M, n):
    worst = {"y": 0.0, "grad": 0.0}
    for C in (32, 96, 256):
        case = bn_act_case(M, n, C)
        for res in (False, True):
            for relu in (True, False):
                for training in (True, False):
                    for wide in (False, True):
                        y, got = _bn_act_gpu(L, case, M, n, C, res, relu, training, wide)
                        y_ref, ref, scales = _bn_act_ref(case, res, relu, training, y)
                        ey = (y.cpu().double() - y_ref).abs().max().item()
                        assert ey < 1e-4, (C, res, relu, training, wide, ey)
                        worst["y"] = max(worst["y"], ey)
                        for q, want in ref.items():
                            scale = want.abs().max().item()
                            if n == 2 and training and q.startswith("dz"):
                                scale = scales[q]
                            eg = (got[q].cpu().double() - want).abs().max().item() / max(scale, 1e-30)
                            assert eg < 1e-4, (C, res, relu, training, wide, q, eg)
                            worst["grad"] = max(worst["grad"], eg)
    print(f"[hrnet] bn_act M={M} rows={n} mode {math_mode}: y {worst['y']:.1e} gradients {worst['grad']:.1e}")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_act_skips_null_outputs(L, training):
    case = bn_act_case(3, 65, 96)
    _, full = _bn_act_gpu(L, case, 3, 65, 96, True, True, training, True)
    _, part = _bn_act_gpu(L, case, 3, 65, 96, True, True, training, True, skip=True)
    assert part["dr"] is None and part["dz2"] is None and part["dgamma0"] is None and part["dbeta2"] is None
    for q, v in part.items():
        assert v is None or torch.equal(v, full[q]), q


# ------------------------------------------------------------------------------------------------------
# HRBasicBlock
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_block_against_float64_and_sparse_basic_block(L, math_mode, training):
    from csn_amd import HRBasicBlock, SparseBasicBlock, build_kernel_map
    coords, p, x, dy = R.block_case()
    g, _ = R.geometry("s1", coords)
    kmap = build_kernel_map(torch.tensor(coords)).to("cuda")
    blk, old = HRBasicBlock(64, 64).cuda().train(training), SparseBasicBlock(64, 64).cuda().train(training)
    blk.load_state_dict(p, strict=False)                                   # (the case holds no num_batches_tracked)
    old.load_state_dict(blk.state_dict())
    xg = x.cuda().requires_grad_(True)
    trace = {}
    y = blk(xg, kmap, trace, "")
    y.backward(dy.cuda())
    masks = (trace["norm1"].cpu() > 0, trace["norm2"].cpu() > 0)
    p64 = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p.items()}
    x64 = x.double().requires_grad_(True)
    y_true, a1, a2 = R.block(g, x64, p64, training)
    y_m, _, _ = R.block(g, x64, p64, training, masks=masks)
    names = [k for k, v in p64.items() if v.requires_grad]
    grads = torch.autograd.grad(y_m, [x64] + [p64[k] for k in names], dy.double())
    ey = (y.detach().cpu().double() - y_true.detach()).abs().max().item()
    got = {"x": xg.grad, **{k: dict(blk.named_parameters())[k].grad for k in names}}
    eg = max((got[k].cpu().double() - w).abs().max().item() / w.abs().max().item() for k, w in zip(["x"] + names, grads))
    with torch.no_grad():
        e_old = (old(x.cuda(), kmap) - y).abs().max().item()
    print(f"[hrnet] block {'train' if training else 'eval'} mode {math_mode}: y {ey:.1e} gradients {eg:.1e} vs SparseBasicBlock {e_old:.1e}")
    assert ey < 1e-4 and eg < 1e-4 and e_old < 2e-4
    for m, a in zip(masks, (a1, a2)):                                      # the masks where float64 decides them
        sure = a.detach().abs() >= 1e-4
        assert bool(((a.detach() > 0) == m)[sure].all())
    if training:
        assert int(blk.norm1.num_batches_tracked) == 1 and int(blk.norm2.num_batches_tracked) == 1
        s = H.stats(R.fwd(g, x, p["conv1.kernel"]), running_mean=p["norm1.running_mean"], running_var=p["norm1.running_var"])
        assert (blk.norm1.running_mean.cpu().double() - s["running_mean"]).abs().max() < 1e-4
        assert (blk.norm1.running_var.cpu().double() - s["running_var"]).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------------
# HRNetBackbone
# ------------------------------------------------------------------------------------------------------
def _points(net, case):
    return R.random_set(300) if case == "rand300" else H.two_coarse_rows(NETS[net][0])


@functools.lru_cache(maxsize=None)
def _backbone_inputs(net, case):
    pts = _points(net, case)
    # the tiny case's maps hold a few hundred elements, where ONE value within 1e-4 of zero is already 0.2 %: its colours are drawn
    # from the first seed at which the float64 restatement's masks are decided (tests/test_cpu_hrnet.py asserts it)
    g = torch.Generator().manual_seed(len(pts) + (4 if case == "coarse2" else 0))
    S, ff = NETS[net]
    return pts, H.Pyramid(pts, S), torch.randn(len(pts), 3, generator=g), torch.randn(len(pts), 32 + 32 * ff * (2 ** S - 1), generator=g)


@functools.lru_cache(maxsize=None)
def backbone_reference(net, case, training):
    """(rows, pre-activations, new running statistics) of the float64 restatement with true ReLUs; shared, never modified."""
    S, ff = NETS[net]
    _, pyr, feats, _ = _backbone_inputs(net, case)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in H.params(S, ff).items()}
    with torch.no_grad():
        rows, pre, new = H.backbone(pyr, feats.double(), p, S, training)
    return rows, pre, new


def _masked_gradients(net, case, training, masks):
    S, ff = NETS[net]
    _, pyr, feats, dy = _backbone_inputs(net, case)
    p = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in H.params(S, ff).items()}
    f64 = feats.double().requires_grad_(True)
    rows, _, _ = H.backbone(pyr, f64, p, S, training, masks=masks)
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    grads = torch.autograd.grad(rows, [f64] + [p[k] for k in names], dy.double())
    return dict(zip(["feats"] + names, grads))


def _run_backbone(net, case, training, fused):
    from csn_amd import HRNetBackbone, build_pyramid
    S, ff = NETS[net]
    pts, _, feats, dy = _backbone_inputs(net, case)
    bb = HRNetBackbone(3, S, ff, fused=fused).cuda().train(training)
    bb.load_state_dict(H.params(S, ff))
    pyr = build_pyramid(torch.tensor(pts), S).to("cuda")
    x = feats.cuda().requires_grad_(True)
    trace = {}
    rows = bb(x, pyr, trace)
    rows.backward(dy.cuda())
    ref_rows, pre, new = backbone_reference(net, case, training)
    assert sorted(trace) == sorted(pre)
    want = _masked_gradients(net, case, training, {k: v.cpu() > 0 for k, v in trace.items()})
    got = {"feats": x.grad, **{k: v.grad for k, v in bb.named_parameters()}}
    assert sorted(got) == sorted(want) and all(v is not None for v in got.values())
    e = {"y": (rows.detach().cpu().double() - ref_rows).abs().max().item()}
    e["grad"] = max((got[k].cpu().double() - w).abs().max().item() / max(w.abs().max().item(), 1e-300) for k, w in want.items())
    e["grad_at"] = max(want, key=lambda k: (got[k].cpu().double() - want[k]).abs().max().item() / max(want[k].abs().max().item(), 1e-300))
    sd = bb.state_dict()
    e["running"] = 0.0
    for name, (rm, rv) in new.items():
        e["running"] = max(e["running"], (sd[name + ".running_mean"].cpu().double() - rm).abs().max().item(),
                           (sd[name + ".running_var"].cpu().double() - rv).abs().max().item())
        assert int(sd[name + ".num_batches_tracked"]) == (1 if training else 0), name
    return e


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_against_float64(L, math_mode, net, case, training):
    base = _run_backbone(net, case, training, fused=False)
    got = _run_backbone(net, case, training, fused=True)
    print(f"[hrnet] backbone {net} {case} {'train' if training else 'eval'} mode {math_mode}: "
          f"fused y {got['y']:.1e} gradients {got['grad']:.1e} ({got['grad_at']}) running {got['running']:.1e} | "
          f"unfused y {base['y']:.1e} gradients {base['grad']:.1e} ({base['grad_at']}) running {base['running']:.1e}")
    for q in ("y", "grad", "running"):
        assert got[q] <= max(1e-4, 2 * base[q]), (q, got[q], base[q])


# ------------------------------------------------------------------------------------------------------
# HRNetSimCSN3S
# ------------------------------------------------------------------------------------------------------
def _batch(seed):
    pts = sorted(R.random_set(300, seed=seed), key=lambda c: c[0])          # rows sorted by shape, any order inside a shape
    g = torch.Generator().manual_seed(50 + seed)
    return torch.tensor(pts), torch.randn(len(pts), 3, generator=g).cuda()


@pytest.mark.parametrize("K", [0, 1])
def test_simcsn3s(L, math_mode, K):
    from csn_amd import HRNetSimCSN3S, build_pyramid
    from csn_amd.minkowski_csn import offsets_from_batch_index
    torch.manual_seed(4)
    model = HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda()
    assert model.backbone.out_channels == 480 and model.head.fc_layer[0].in_features == 480
    q = _batch(0)
    keys = [_batch(1)] if K else None
    # eval: the logits are the head's own on the backbone's rows — the same bits
    model.eval()
    with torch.no_grad():
        logits = model(q, keys)
        rows = [model.backbone(f, build_pyramid(c, 3).to("cuda")) for c, f in [q] + (keys or [])]
        offs = [offsets_from_batch_index(c[:, 0]) for c, _ in [q] + (keys or [])]
        again = model.head(rows[0], offs[0], keys=[(rows[1], offs[1])] if K else None)
        ssa = model(q, keys, return_ssa=True)
    assert logits.shape == (q[0].shape[0], 6) and torch.equal(logits, again)
    assert ssa.shape == (q[0].shape[0], 64) and bool(torch.isfinite(ssa).all())
    # train: every parameter receives a gradient; every BatchNorm saw K + 1 batches, in order
    model.train()
    stem = model.backbone.bn0s1
    rm0 = stem.running_mean.clone().cpu().double()
    model(q, keys).square().mean().backward()
    unused = ("head.linear_q.weight", "head.linear_k.weight") if K == 0 else ()
    for name, prm in model.named_parameters():
        if name in unused:
            continue
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0, name
    for name, buf in model.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(buf) == K + 1, name
    want, w = rm0, model.backbone.conv0s1.kernel.detach().cpu()
    for c, f in [q] + (keys or []):
        z = R.fwd(R.geometry("s1", c.tolist(), k=5)[0], f.cpu(), w)
        want = (1 - 0.02) * want + 0.02 * z.mean(0)
    err = (stem.running_mean.cpu().double() - want).abs().max().item()
    print(f"[hrnet] HRNetSimCSN3S K={K} mode {math_mode}: stem running mean after {K + 1} batches {err:.1e}")
    assert err < 1e-4
