"""GPU parity of the sparse 3D convolution on voxel rows (csn_amd/csrc/sparse_conv.hip; include/csn_hip.h section 14;
csn_amd/minkowski_conv.py) against the float64 restatement tests/sparse_conv_ref.py, in math modes 0 and 1: the raw ABI on point
sets chosen for the places the kernel can go wrong (a single voxel, a dense 4^3 block, random occupancy 0.15 trimmed to 31 / 33 /
129 / 1031 rows — either side of the 32-row wave and 128-row work-group tiles — and two far-apart clusters followed by isolated
voxels, where whole tiles skip most offsets) at every width pair, at natural and at padded pitches; stride 2 and the transposed
form, one shared map through ``transpose()``; every kernel instance (the column blocks a wave owns pinned by ``CSN_DEV_SCONV_NB``)
and the launch rule's own choice at 32768 rows; the stride-1 backward on the reversed forward table; determinism; NULL outputs; the padded stem and ``SparseBasicBlock`` through autograd.
(The random sets sit on a 12^3 grid up to 129 rows; 0.15 of two 12^3 grids is about 518 voxels, so the 1031-row set sits on 16^3.)

Bounds (the project's contract): outputs within 1e-4 absolute (weights of variance 1 / (KV c_in): outputs are O(1)); each gradient
within 1e-4 of its tensor's max.  The block's outputs and ReLU masks are compared where the float64 pre-activation is at least 1e-4
from zero (at most 0.1 % of the elements may be nearer: tests/test_cpu_sparse_conv.py asserts that on the reference alone); its
gradients are taken against the float64 composition under the GPU's own two ReLU masks.

Measured on MI355X, maxima over the cases (fp32 / bf16x3): raw ABI at stride 1, all point sets
and widths: y 1.2e-5 (dense 4^3, 256 -> 256) / 1.9e-5, dx 3.7e-6 / 6.3e-6, dw 3.2e-7 / 1.2e-5 (the single voxel), dbias 5.0e-8 / 5.0e-8;
the longest contraction (27 x 256 terms, 256 -> 256) stays inside the bound in bf16x3 against each tensor's max, so no case needs the
absolute-value scale.  Stride 2 and transposed: y 2.1e-6 / 9.6e-6, dx 8.8e-7 / 4.8e-6, dw 1.1e-7 / 5.3e-6, dbias 3.5e-8.  Down + up on
one map: y 1.1e-6 / 5.1e-6, gradients <= 1.1e-6 / 7.3e-6.  Stem: y 4.8e-7 / 8.6e-6, gradients <= 7.6e-7 / 4.8e-6.  Block: y 3.2e-6 /
4.6e-5 (training mode), every gradient <= 4.2e-7 / 8.1e-6.  Column blocks per wave pinned to 2 / 3 / 4 (1031 rows, 64 ... 256 columns):
y 3.8e-6 / 1.2e-5, dx 1.3e-6 / 5.4e-6, dw 4.7e-7 / 5.1e-6, dbias 4.9e-8.  The launch rule at 32768 rows (64, 128, 256 wide): y 5.8e-6 /
1.4e-5, dx 2.1e-6 / 4.9e-6, dw 1.8e-6 / 5.0e-6, dbias 5.4e-8."""
import functools

import pytest
import torch

from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
NB_CASES = [(64, 64, 2), (96, 96, 3), (128, 128, 4), (160, 160, 3), (160, 96, 4), (192, 224, 3), (256, 256, 4), (224, 192, 4)]
SETS = {"rand32768": lambda: R.random_set(32768), "single": R.single_voxel, "dense4": R.dense_block, "rand31": lambda: R.random_set(31), "rand33": lambda: R.random_set(33),
        "rand129": lambda: R.random_set(129), "rand1031": lambda: R.random_set(1031), "clusters": R.two_clusters}
WIDTHS = [(32, 32, 3), (64, 64, 3), (32, 64, 3), (128, 128, 3), (256, 256, 3), (32, 32, 5)]


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


@functools.lru_cache(maxsize=None)
def _geometry(mode, name, k):
    """Dictionary geometry, the kernel map built on CPU tensors, and the coordinate lists of one case (shared, never modified).
    mode "s2": from the set onto its coarse set; "tr": from that coarse set back onto the set."""
    from csn_amd.minkowski_conv import build_kernel_map
    pts = SETS[name]()
    if mode == "s1":
        g, _ = R.geometry("s1", pts, k=k)
        return g, build_kernel_map(torch.tensor(pts), kernel_size=k)
    down = build_kernel_map(torch.tensor(pts), kernel_size=3, stride=2)
    if mode == "s2":
        return R.geometry("s2", pts)[0], down
    return R.geometry("tr", R.down_coords([tuple(c) for c in pts], 1), fine=pts)[0], down.transpose()


@functools.lru_cache(maxsize=None)
def _case(mode, name, c_in, c_out, k):
    """Inputs and the float64 forward and backward of one case, computed once and shared between the math modes."""
    g, m = _geometry(mode, name, k)
    t = R.tensors(len(name) + c_in + 3 * c_out + k, g.n_in, g.n_out, g.KV, c_in, c_out)
    return g, m, t, R.fwd(g, t["x"], t["w"], t["b"]), R.bwd(g, t["dy"], t["x"], t["w"])


def _rows(t, pad, fill):
    """(n, c) CPU tensor -> a device view of pitch c + pad whose padding holds ``fill``; with pad the view starts 16 bytes into
    its buffer (16-byte aligned, not 64)."""
    n, c = t.shape
    if not pad:
        return t.cuda().contiguous(), None
    buf = torch.full((4 + n * (c + pad),), fill, dtype=torch.float32, device="cuda")
    view = buf[4:].view(n, c + pad)
    view[:, :c] = t.cuda()
    return view[:, :c], buf


def _pad_intact(buf, n, c, pad, fill):
    return bool((buf[:4] == fill).all()) and bool((buf[4:].view(n, c + pad)[:, c:] == fill).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


class Run:
    """One forward (+ backward) through the raw ABI."""

    def __init__(self, L, m, t, pad=0, bias=True, explicit_bwd=False):
        lib = L.lib()
        self.explicit_bwd = explicit_bwd
        self.L, self.m, self.pad = L, m.to("cuda"), pad
        self.KV, self.c_in, self.c_out = t["w"].shape
        self.n_in, self.n_out = m.n_in, m.n_out
        self.x, self.xbuf = _rows(t["x"], pad, 1e30)
        self.w = t["w"].cuda().contiguous()
        self.b = t["b"].cuda().contiguous() if bias else None
        self.y, self.ybuf = _rows(torch.zeros(self.n_out, self.c_out), pad, CANARY)
        if not pad:
            self.y.fill_(CANARY)
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.csn_sparse_conv_fwd_f32(_ptr(self.x), self.c_in + pad, self.n_in, _ptr(self.m.fwd), self.n_out, self.KV, self.c_in,
                                            self.c_out, _ptr(self.w), _ptr(self.b), _ptr(self.y), self.c_out + pad, st), "fwd")

    def backward(self, dy_cpu, want=("dx", "dw", "dbias")):
        lib, pad = self.L.lib(), self.pad
        self.dy, self.dybuf = _rows(dy_cpu, pad, 1e30)
        self.dx, self.dxbuf = _rows(torch.zeros(self.n_in, self.c_in), pad, CANARY)
        if not pad:
            self.dx.fill_(CANARY)
        self.dw = torch.full((self.KV, self.c_in, self.c_out), CANARY, device="cuda")
        self.dbias = torch.full((self.c_out,), CANARY, device="cuda")
        wb = lib.csn_sparse_conv_workspace_bytes(self.n_in, self.n_out, self.KV, self.c_in, self.c_out, 1)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        # a stride-1 map keeps no second table: NULL makes the kernel walk fwd in reversed offset order
        self.bwd_table = self.m.bwd if self.explicit_bwd else self.m.bwd_table
        st = torch.cuda.current_stream().cuda_stream
        self.L.check(lib.csn_sparse_conv_bwd_f32(_ptr(self.dy), self.c_out + pad, _ptr(self.x), self.c_in + pad, self.n_in, self.n_out,
                                                 self.KV, self.c_in, self.c_out, _ptr(self.m.fwd), _ptr(self.bwd_table), _ptr(self.w),
                                                 _ptr(self.dx) if "dx" in want else None, self.c_in + pad,
                                                 _ptr(self.dw) if "dw" in want else None,
                                                 _ptr(self.dbias) if "dbias" in want else None, _ptr(ws), wb, st), "bwd")
        return self


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


def _check(tag, run, f, b):
    """y within 1e-4 absolute, every gradient within 1e-4 of its tensor's max; prints and returns the figures."""
    e = {"y": _err(run.y, f)}
    for k in ("dx", "dw", "dbias"):
        e[k] = _err(getattr(run, k), b[k]) / max(b[k].abs().max().item(), 1e-30)
    print(f"[sparse_conv] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    for k in ("y", "dx", "dw", "dbias"):
        assert torch.isfinite(getattr(run, k)).all(), k
    assert max(e.values()) < 1e-4, e
    return e


@pytest.mark.parametrize("c_in,c_out,k", WIDTHS, ids=[f"{a}to{b}k{k}" for a, b, k in WIDTHS])
@pytest.mark.parametrize("name", [n for n in SETS if n != "rand32768"])
def test_raw_abi_against_float64(L, math_mode, name, c_in, c_out, k):
    g, m, t, f, b = _case("s1", name, c_in, c_out, k)
    run = Run(L, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {name} n {g.n_in} {c_in}->{c_out} k{k}", run, f, b)


@pytest.mark.parametrize("name", [n for n in SETS if n != "rand32768"])
def test_padded_pitches_and_offset_bases_leave_the_canary(L, math_mode, name):
    c_in, c_out, k = WIDTHS[0]
    g, m, t, f, b = _case("s1", name, c_in, c_out, k)
    run = Run(L, m, t, pad=4).backward(t["dy"])
    _check(f"mode {math_mode} {name} n {g.n_in} {c_in}->{c_out} k{k} padded", run, f, b)
    assert _pad_intact(run.ybuf, g.n_out, c_out, 4, CANARY) and _pad_intact(run.dxbuf, g.n_in, c_in, 4, CANARY)
    assert _pad_intact(run.xbuf, g.n_in, c_in, 4, 1e30) and _pad_intact(run.dybuf, g.n_out, c_out, 4, 1e30)
    plain = Run(L, m, t).backward(t["dy"])
    for key in ("y", "dx", "dw", "dbias"):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key          # the pitch changes no bit


@pytest.mark.parametrize("c_in,c_out,nb", NB_CASES, ids=[f"{a}to{b}nb{n}" for a, b, n in NB_CASES])
def test_every_column_block_count_against_float64(L, math_mode, c_in, c_out, nb):
    """The launch rule gives a wave 2, 3 or 4 column blocks only from 16257 / 32641 rows up; CSN_DEV_SCONV_NB pins the count, so
    the 1031-row set reaches every instance of the forward (blocks of c_out) and of dx (blocks of c_in): one and two column
    groups, and a last group with 1, 2 or 3 blocks past the width.  The pinned launches give the bits of the launch rule's own."""
    g, m, t, f, b = _case("s1", "rand1031", c_in, c_out, 3)
    lib = L.lib()
    assert lib.csn_dev_set(L.DEV_SCONV_NB, 5) == -1 and lib.csn_dev_get(L.DEV_SCONV_NB) == 0
    plain = Run(L, m, t).backward(t["dy"])
    assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) == 0
    try:
        run = Run(L, m, t).backward(t["dy"])
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    _check(f"mode {math_mode} nb {nb} n {g.n_in} {c_in}->{c_out}", run, f, b)
    for key in ("y", "dx"):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key


@pytest.mark.parametrize("c_in,c_out", [(64, 64), (128, 128), (256, 256)], ids=["64to64", "128to128", "256to256"])
def test_launch_rule_at_full_size_against_float64(L, math_mode, c_in, c_out):
    """32768 voxels: the row count of the HRNet3S top level, where the launch rule itself gives a wave 2 (64 wide) and 4 (128 and, in two column groups, 256
    wide) column blocks, and the weight gradient several split-K chunks."""
    g, m, t, f, b = _case("s1", "rand32768", c_in, c_out, 3)
    assert L.lib().csn_dev_get(L.DEV_SCONV_NB) == 0
    run = Run(L, m, t).backward(t["dy"])
    _check(f"mode {math_mode} rule n {g.n_in} {c_in}->{c_out}", run, f, b)


def test_reversed_forward_table_equals_an_explicit_backward_table(L, math_mode):
    g, m, t, _, _ = _case("s1", "rand1031", 64, 64, 3)
    assert m.bwd_table is None
    a = Run(L, m, t).backward(t["dy"], want=("dx",))
    b = Run(L, m, t, explicit_bwd=True).backward(t["dy"], want=("dx",))
    assert torch.equal(a.dx, b.dx)


@pytest.mark.parametrize("c_in,c_out", [(64, 128), (128, 64)], ids=["64to128", "128to64"])
@pytest.mark.parametrize("mode", ["s2", "tr"])
def test_stride_2_and_transposed_against_float64(L, math_mode, mode, c_in, c_out):
    g, m, t, f, b = _case(mode, "rand1031", c_in, c_out, 3)
    assert m.transposed == (mode == "tr") and (g.n_in, g.n_out) == (m.n_in, m.n_out) and g.n_in != g.n_out
    run = Run(L, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {mode} {g.n_in}->{g.n_out} rows {c_in}->{c_out}", run, f, b)


def test_map_built_on_the_device_equals_the_cpu_map(L):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = torch.tensor(SETS["rand1031"]())
    for kw in (dict(kernel_size=5), dict(kernel_size=3, stride=2)):
        a, b = build_kernel_map(pts, **kw), build_kernel_map(pts.cuda(), **kw)
        assert b.fwd.is_cuda and torch.equal(a.fwd, b.fwd.cpu()) and torch.equal(a.bwd, b.bwd.cpu())
        assert torch.equal(a.out_coords, b.out_coords.cpu())


def test_down_and_up_share_one_map_through_autograd(L, math_mode):
    """x -> stride-2 convolution -> transposed convolution back onto x's coordinates, both on ONE map (``transpose()``): outputs and
    the gradients to x and to both kernels against the float64 composition."""
    from csn_amd import sparse_conv3d
    gd, m = _geometry("s2", "rand1031", 3)
    gu, _ = _geometry("tr", "rand1031", 3)
    t = R.tensors(77, gd.n_in, gd.n_in, 27, 64, 128)
    wu = R.tensors(78, 1, 1, 27, 128, 64)["w"]
    dy = R.tensors(79, gd.n_in, 1, 1, 64, 1)["x"]
    x64, wd64, wu64 = (v.double().requires_grad_(True) for v in (t["x"], t["w"], wu))
    ref = R._conv_autograd(gu, R._conv_autograd(gd, x64, wd64), wu64)
    (ref * dy.double()).sum().backward()
    md = m.to("cuda")
    x, wd, wuu = (v.cuda().requires_grad_(True) for v in (t["x"], t["w"], wu))
    y = sparse_conv3d(sparse_conv3d(x, wd, None, md), wuu, None, md.transpose())
    (y * dy.cuda()).sum().backward()
    e = {"y": _err(y, ref.detach())}
    for k, got, want in (("dx", x.grad, x64.grad), ("dw_down", wd.grad, wd64.grad), ("dw_up", wuu.grad, wu64.grad)):
        e[k] = _err(got, want) / want.abs().max().item()
    print(f"[sparse_conv] mode {math_mode} down+up: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e


def test_two_calls_give_the_same_bits(L, math_mode):
    for mode, name, c_in, c_out in (("s1", "rand1031", 256, 256), ("s2", "rand1031", 64, 128)):
        g, m, t, _, _ = _case(mode, name, c_in, c_out, 3)
        a = Run(L, m, t).backward(t["dy"])
        b = Run(L, m, t).backward(t["dy"])
        for k in ("y", "dx", "dw", "dbias"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (mode, k)


def test_null_outputs_are_skipped(L, math_mode):
    g, m, t, f, _ = _case("s1", "rand129", 64, 64, 3)
    full = Run(L, m, t).backward(t["dy"])
    for skip in ("dx", "dw", "dbias"):
        want = tuple(k for k in ("dx", "dw", "dbias") if k != skip)
        part = Run(L, m, t).backward(t["dy"], want=want)
        assert bool((getattr(part, skip) == CANARY).all()), skip
        for k in want:
            assert torch.equal(getattr(part, k), getattr(full, k)), (skip, k)
    none = Run(L, m, t).backward(t["dy"], want=())
    assert all(bool((getattr(none, k) == CANARY).all()) for k in ("dx", "dw", "dbias"))
    nobias = Run(L, m, t, bias=False)                                   # bias NULL: y without it
    assert _err(nobias.y, f - t["b"].double()) < 1e-4


# ------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------
def test_padded_stem_through_autograd(L, math_mode):
    """``SparseConv3d(3, 32, kernel_size=5)``: 3 colour channels zero-padded to 32 in the wrapper, gradients sliced back."""
    from csn_amd import SparseConv3d
    g, m = _geometry("s1", "rand1031", 5)
    t = R.tensors(91, g.n_in, g.n_out, 125, 3, 32)
    f, b = R.fwd(g, t["x"], t["w"], t["b"]), R.bwd(g, t["dy"], t["x"], t["w"])
    stem = SparseConv3d(3, 32, kernel_size=5, bias=True)
    with torch.no_grad():
        stem.kernel.copy_(t["w"]); stem.bias.copy_(t["b"][None])
    stem = stem.cuda()
    x = t["x"].cuda().requires_grad_(True)
    y = stem(x, m.to("cuda"))
    (y * t["dy"].cuda()).sum().backward()
    assert y.shape == (g.n_out, 32) and x.grad.shape == (g.n_in, 3) and stem.kernel.grad.shape == (125, 3, 32)
    assert stem.bias.grad.shape == (1, 32)
    e = {"y": _err(y, f), "dx": _err(x.grad, b["dx"]) / b["dx"].abs().max().item(),
         "dw": _err(stem.kernel.grad, b["dw"]) / b["dw"].abs().max().item(),
         "dbias": _err(stem.bias.grad[0], b["dbias"]) / b["dbias"].abs().max().item()}
    print(f"[sparse_conv] mode {math_mode} stem: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e
    # no gradient asked of the rows: dx is skipped, the kernel's gradient is the same bits
    dw = stem.kernel.grad.clone()
    stem.zero_grad()
    (stem(t["x"].cuda(), m.to("cuda")) * t["dy"].cuda()).sum().backward()
    assert torch.equal(stem.kernel.grad, dw)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_basic_block_through_autograd(L, math_mode, training):
    from csn_amd import SparseBasicBlock, build_kernel_map
    coords, p, x_cpu, dy = R.block_case()
    g, _ = R.geometry("s1", coords)
    names = [n for n in p if "running" not in n]
    p64 = {n: (v.double().requires_grad_(True) if n in names else v.double()) for n, v in p.items()}
    x64 = x_cpu.double().requires_grad_(True)
    with torch.no_grad():
        ref, a1, a2 = R.block(g, x64, p64, training)

    blk = SparseBasicBlock(64, 64, bn_momentum=0.02)
    missing = blk.load_state_dict(p, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys
    blk = blk.cuda().train(training)
    seen = {}
    hook = blk.norm1.register_forward_hook(lambda mod, inp, out: seen.__setitem__("a1", out.detach()))
    m = build_kernel_map(torch.tensor(coords).cuda(), kernel_size=3)
    x = x_cpu.cuda().requires_grad_(True)
    y = blk(x, m)
    hook.remove()
    (y * dy.cuda()).sum().backward()
    assert int(blk.norm1.num_batches_tracked) == (1 if training else 0)

    m1, m2 = seen["a1"].cpu() > 0, y.detach().cpu() > 0
    for a, mask in ((a1, m1), (a2, m2)):
        decided = a.abs() >= 1e-4
        assert 1.0 - decided.double().mean().item() <= 1e-3
        assert torch.equal(mask[decided], (a > 0)[decided])
    decided = a2.abs() >= 1e-4
    e = {"y": (y.detach().cpu().double() - ref)[decided].abs().max().item()}
    # the gradients under the GPU's own two ReLU masks
    ym, _, _ = R.block(g, x64, p64, training, masks=(m1, m2))
    (ym * dy.double()).sum().backward()
    got = {n: prm.grad for n, prm in blk.named_parameters()}
    assert sorted(got) == sorted(names)
    e["dx"] = _err(x.grad, x64.grad) / x64.grad.abs().max().item()
    for n in names:
        e[n] = _err(got[n], p64[n].grad) / p64[n].grad.abs().max().item()
    print(f"[sparse_conv] mode {math_mode} block {'train' if training else 'eval'}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e
