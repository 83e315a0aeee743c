"""GPU parity of the kernel-2 stride-2 convolution and its transposed form (csn_amd/csrc/octant_conv.hip; include/csn_hip.h section
21; csn_amd/minkowski_conv.py) against the float64 restatement tests/octant_ref.py, in math modes 0 and 1: the raw ABI in both
directions on point sets chosen for the places the kernels can go wrong — a single voxel, a dense 4^3 block (all 8 children
everywhere), random occupancy trimmed to 33 / 129 / 1031 rows (octant segments of 1-8, 7-23 and 115-142 rows: below, and across, the
128-row tile), two clusters and a line (one segment of 180 rows, seven of 9-27), their level 3 (four EMPTY octants) and a set whose
y are all even (four empty octants) — at four width pairs, at natural and padded pitches; every kernel instance (the column blocks a
wave owns pinned by ``CSN_DEV_SCONV_NB``); NULL outputs; determinism; the two autograd nodes and their composition on one map;
``cat_conv3d`` against the convolution of the concatenation.  The weight gradient past one 16-row step per wave: widths (160, 256),
(224, 256) and (256, 256) on 1031 and 2100 rows, whose split-K chunks are 128, 192 and 256 rows (every other case here has chunk 64: one
step, the prefetch of the next never runs), with two calls of the chunk-192 case compared bit for bit; and two sets whose segments fill
the 128-row tile exactly (eight of 128 rows) or straddle it by one row (129, six of 128, 127).

Bounds (the project's contract, as tests/test_gpu_sparse_conv.py states it): weights of variance 1 / (8 c_in), outputs within 1e-4
absolute, each gradient within 1e-4 of its tensor's max.  The contraction is 8 x 256 terms at most — shorter than the 27 x 256 that
already holds the bound.

Measured on MI355X, maxima over the cases (fp32 / bf16x3).  Raw ABI, all point sets and widths, down: y 4.8e-6 / 1.7e-5, dx 7.1e-7 /
8.8e-6, dw 1.8e-7 / 1.4e-5, dbias 5.4e-8; up: y 1.2e-6 / 1.3e-5, dx 1.6e-6 / 1.0e-5, dw 1.6e-7 / 1.0e-5, dbias 4.3e-8.  Padded pitches:
y 2.7e-6 / 1.5e-5, gradients <= 1.0e-6 / 1.0e-5.  Column blocks per wave pinned to 2 / 3 / 4 on 1031 rows: y 4.1e-6 / 1.5e-5, dx 1.1e-6 /
6.5e-6, dw 1.5e-7 / 5.9e-6.  Autograd nodes: y 1.5e-6 / 1.1e-5, gradients <= 6.4e-7 / 6.5e-6.  Down + up on one map: y 3.8e-7 / 6.5e-6,
gradients <= 2.9e-7 / 7.0e-6.  ``cat_conv3d``: y 2.3e-6 / 7.7e-6, dx 1.1e-6 / 5.0e-6, dw 1.5e-7 / 5.2e-6.  Chunks of 128 / 192 / 256 rows, down:
y 2.6e-6 / 1.2e-5, dx 8.8e-7 / 5.4e-6, dw 2.6e-7 / 5.3e-6, dbias 4.1e-8; up: y 1.2e-6 / 9.8e-6, dx 1.2e-6 / 5.2e-6, dw 2.0e-7 / 5.5e-6, dbias
3.3e-8.  Exactly full tiles, down: y 6.8e-6 / 2.0e-5, dx 6.4e-7 / 7.4e-6, dw 1.4e-7 / 5.4e-6; up: y 1.2e-6 / 9.3e-6, dx 2.1e-6 / 4.6e-6, dw 1.3e-7 /
5.5e-6."""
import functools

import pytest
import torch

from tests import octant_ref as O
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
SETS = {"single": (R.single_voxel, 1), "dense4": (R.dense_block, 1), "rand33": (lambda: R.random_set(33), 1),
        "rand129": (lambda: R.random_set(129), 1), "rand1031": (lambda: R.random_set(1031), 1), "clusters": (R.two_clusters, 1),
        "clusters_l3": (lambda: O.level(R.two_clusters(), 1, 3)[0], 8), "even_y": (O.even_y, 1)}
# beyond the sets every test walks: segments of exactly 128 rows, 129 / 127 rows side by side, and one large enough for weight-gradient
# chunks of 192 and 256 rows (the cases of O.WGRAD_CASES)
MORE_SETS = {"box128": (O.box128, 1), "box127_129": (O.box127_129, 1), "rand2100": (O.WGRAD_SETS["rand2100"], 1)}
WIDTHS = [(32, 32), (96, 64), (64, 96), (256, 256)]
NB_CASES = [(64, 64, 2), (96, 96, 3), (128, 128, 4), (256, 256, 4), (256, 96, 3), (96, 256, 2)]


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
def _geometry(name):
    """Dictionary partition and the octant map built on CPU tensors of one point set (shared, never modified)."""
    from csn_amd.minkowski_conv import build_octant_map
    make, ts = (SETS.get(name) or MORE_SETS[name])
    pts = make()
    return O.Partition(pts, ts), build_octant_map(torch.tensor(pts), tensor_stride=ts)


@functools.lru_cache(maxsize=None)
def _case(up, name, c_in, c_out):
    """Inputs and the float64 forward and backward of one case, computed once and shared between the math modes."""
    p, m = _geometry(name)
    n_in, n_out = (p.n_coarse, p.n_fine) if up else (p.n_fine, p.n_coarse)
    t = O.tensors(len(name) + c_in + 3 * c_out + int(up), n_in, n_out, c_in, c_out)
    f = (O.up_fwd if up else O.down_fwd)(p, t["x"], t["w"], t["b"])
    b = (O.up_bwd if up else O.down_bwd)(p, t["dy"], t["x"], t["w"])
    return p, m, t, f, b


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
    """One forward (+ backward) of one direction through the raw ABI."""

    def __init__(self, L, up, m, t, pad=0, bias=True):
        lib = L.lib()
        self.L, self.up, self.m, self.pad = L, up, m.to("cuda"), pad
        _, self.c_in, self.c_out = t["w"].shape
        self.n_fine, self.n_coarse = m.n_fine, m.n_coarse
        self.n_in, self.n_out = (self.n_coarse, self.n_fine) if up else (self.n_fine, self.n_coarse)
        self.x, self.xbuf = _rows(t["x"], pad, 1e30)
        self.w = t["w"].cuda().contiguous()
        self.b = t["b"].cuda().contiguous() if bias else None
        self.y, self.ybuf = _rows(torch.zeros(self.n_out, self.c_out), pad, CANARY)
        if not pad:
            self.y.fill_(CANARY)
        st = torch.cuda.current_stream().cuda_stream
        mm = self.m
        if up:
            L.check(lib.csn_octant_up_fwd_f32(_ptr(self.x), self.c_in + pad, self.n_coarse, _ptr(mm.parent), _ptr(mm.order), _ptr(mm.seg),
                                              self.n_fine, self.c_in, self.c_out, _ptr(self.w), _ptr(self.b), _ptr(self.y),
                                              self.c_out + pad, st), "up fwd")
        else:
            L.check(lib.csn_octant_down_fwd_f32(_ptr(self.x), self.c_in + pad, self.n_fine, _ptr(mm.children), self.n_coarse, self.c_in,
                                                self.c_out, _ptr(self.w), _ptr(self.b), _ptr(self.y), self.c_out + pad, st), "down fwd")

    def backward(self, dy_cpu, want=("dx", "dw", "dbias")):
        lib, pad, mm = self.L.lib(), self.pad, self.m
        self.dy, self.dybuf = _rows(dy_cpu, pad, 1e30)
        self.dx, self.dxbuf = _rows(torch.zeros(self.n_in, self.c_in), pad, CANARY)
        if not pad:
            self.dx.fill_(CANARY)
        self.dw = torch.full((8, self.c_in, self.c_out), CANARY, device="cuda")
        self.dbias = torch.full((self.c_out,), CANARY, device="cuda")
        wb = lib.csn_octant_conv_workspace_bytes(self.n_fine, self.n_coarse, self.c_in, self.c_out, int(self.up), 1)
        assert wb > 0
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        out = (_ptr(self.dx) if "dx" in want else None, self.c_in + pad, _ptr(self.dw) if "dw" in want else None,
               _ptr(self.dbias) if "dbias" in want else None, _ptr(ws), wb, st)
        if self.up:
            self.L.check(lib.csn_octant_up_bwd_f32(_ptr(self.dy), self.c_out + pad, _ptr(self.x), self.c_in + pad, self.n_fine,
                                                   self.n_coarse, self.c_in, self.c_out, _ptr(mm.children), _ptr(mm.parent),
                                                   _ptr(mm.order), _ptr(mm.seg), _ptr(self.w), *out), "up bwd")
        else:
            self.L.check(lib.csn_octant_down_bwd_f32(_ptr(self.dy), self.c_out + pad, _ptr(self.x), self.c_in + pad, self.n_fine,
                                                     self.n_coarse, self.c_in, self.c_out, _ptr(mm.parent), _ptr(mm.order),
                                                     _ptr(mm.seg), _ptr(self.w), *out), "down bwd")
        return self


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


def _figures(got, f, b):
    e = {"y": _err(got["y"], f)}
    for k in ("dx", "dw", "dbias"):
        e[k] = _err(got[k], b[k]) / max(b[k].abs().max().item(), 1e-30)
    return e


def _check(tag, run, f, b):
    """y within 1e-4 absolute, every gradient within 1e-4 of its tensor's max; prints and returns the figures."""
    e = _figures({k: getattr(run, k) for k in ("y", "dx", "dw", "dbias")}, f, b)
    print(f"[octant] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    for k in ("y", "dx", "dw", "dbias"):
        assert torch.isfinite(getattr(run, k)).all(), k
    assert max(e.values()) < 1e-4, e
    return e


DIRS = pytest.mark.parametrize("up", [False, True], ids=["down", "up"])


@DIRS
@pytest.mark.parametrize("c_in,c_out", WIDTHS, ids=[f"{a}to{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("name", list(SETS))
def test_raw_abi_against_float64(L, math_mode, name, c_in, c_out, up):
    p, m, t, f, b = _case(up, name, c_in, c_out)
    run = Run(L, up, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} n {p.n_fine}/{p.n_coarse} {c_in}->{c_out}", run, f, b)
    # an octant without rows has no weight gradient: written, as zeros
    for k, n in enumerate(p.segments()):
        if n == 0:
            assert not run.dw[k].any(), k


def test_the_sets_have_the_segments_the_kernels_are_tested_on():
    seg = lambda name: sorted(_geometry(name)[0].segments())
    assert seg("rand33")[0] >= 1 and seg("rand33")[-1] <= 8
    assert seg("rand129")[0] >= 7 and seg("rand129")[-1] <= 23
    assert seg("rand1031")[0] < 128 < seg("rand1031")[-1]                       # segments on both sides of the 128-row tile
    assert seg("clusters")[-1] == 180 and seg("clusters")[-2] <= 27
    assert seg("clusters_l3").count(0) == 4 and seg("even_y").count(0) == 4
    assert seg("dense4") == [8] * 8
    assert _geometry("box128")[0].segments() == [128] * 8                      # every tile exactly full, the next slot empty
    assert (_geometry("box128")[0].n_fine, _geometry("box128")[0].n_coarse) == (1024, 128)
    assert _geometry("box127_129")[0].segments() == [129, 128, 128, 128, 128, 128, 128, 127]
    assert seg("rand2100")[0] >= 243 and seg("rand2100")[-1] <= 283            # a chunk of 192 or 256 rows and a short one
    assert O.WGRAD_SETS["rand1031"]() == SETS["rand1031"][0]()


WGRAD_IDS = [f"{n}-{a}to{b}-chunk{c}" for n, a, b, c in O.WGRAD_CASES]


@DIRS
@pytest.mark.parametrize("name,c_in,c_out,chunk", O.WGRAD_CASES, ids=WGRAD_IDS)
def test_weight_gradient_past_one_step_per_wave_against_float64(L, math_mode, name, c_in, c_out, chunk, up):
    """The split-K chunk of every case above is 64 rows: a wave contracts 16 rows, one step, and the prefetch of the next step never
    runs.  These widths and sets give chunks of 128, 192 and 256 rows (pinned on the CPU by tests/test_cpu_ragged_head.py): two to
    four steps per wave, a wave that ends inside a later step, waves with nothing, and 5, 7 and 2 row blocks of dw."""
    p, m, t, f, b = _case(up, name, c_in, c_out)
    run = Run(L, up, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} {c_in}->{c_out} chunk {chunk}", run, f, b)
    for key in ("y", "dx", "dw", "dbias"):
        assert not bool((getattr(run, key) == CANARY).any()), key
    if chunk == 192:
        again = Run(L, up, m, t).backward(t["dy"])
        for key in ("y", "dx", "dw", "dbias"):
            assert torch.equal(getattr(run, key), getattr(again, key)), key     # two calls give the same bits


@DIRS
@pytest.mark.parametrize("c_in,c_out", [(96, 64), (256, 256)], ids=["96to64", "256to256"])
@pytest.mark.parametrize("name", ["box128", "box127_129"])
def test_exactly_full_tiles_write_every_row_once(L, math_mode, name, c_in, c_out, up):
    """Segments of exactly 128 rows (a tile exactly full, the slot behind it empty) and of 129 and 127 rows side by side: every output
    row of the one-weight row product is written (no canary left) with the right values, dw[k] of every octant is right."""
    p, m, t, f, b = _case(up, name, c_in, c_out)
    run = Run(L, up, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} n {p.n_fine}/{p.n_coarse} {c_in}->{c_out}", run, f, b)
    for key in ("y", "dx", "dw", "dbias"):
        assert not bool((getattr(run, key) == CANARY).any()), key
    for k in range(8):
        scale = max(b["dw"][k].abs().max().item(), 1e-30)
        assert _err(run.dw[k], b["dw"][k]) < 1e-4 * scale, k                     # each octant against its own maximum


@DIRS
@pytest.mark.parametrize("name", list(SETS))
def test_padded_pitches_and_offset_bases_leave_the_canary(L, math_mode, name, up):
    c_in, c_out = WIDTHS[1]
    p, m, t, f, b = _case(up, name, c_in, c_out)
    run = Run(L, up, m, t, pad=4).backward(t["dy"])
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} {c_in}->{c_out} padded", run, f, b)
    assert _pad_intact(run.ybuf, run.n_out, c_out, 4, CANARY) and _pad_intact(run.dxbuf, run.n_in, c_in, 4, CANARY)
    assert _pad_intact(run.xbuf, run.n_in, c_in, 4, 1e30) and _pad_intact(run.dybuf, run.n_out, c_out, 4, 1e30)
    plain = Run(L, up, m, t).backward(t["dy"])
    for key in ("y", "dx", "dw", "dbias"):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key          # the pitch changes no bit


@DIRS
@pytest.mark.parametrize("c_in,c_out,nb", NB_CASES, ids=[f"{a}to{b}nb{n}" for a, b, n in NB_CASES])
def test_every_column_block_count_against_float64(L, math_mode, c_in, c_out, nb, up):
    """At 1031 rows the launch rule gives a wave one column block (2, 3, 4 and 8 column groups at 64, 96, 128 and 256 columns);
    CSN_DEV_SCONV_NB pins the count, so the same set reaches every instance: one and two column groups, and a last group with
    blocks past the width.  The pinned launches give the bits of the launch rule's own."""
    p, m, t, f, b = _case(up, "rand1031", c_in, c_out)
    lib = L.lib()
    plain = Run(L, up, m, t).backward(t["dy"])
    _check(f"mode {math_mode} {'up' if up else 'down'} rule {c_in}->{c_out}", plain, f, b)
    assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) == 0
    try:
        run = Run(L, up, m, t).backward(t["dy"])
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    _check(f"mode {math_mode} {'up' if up else 'down'} nb {nb} {c_in}->{c_out}", run, f, b)
    for key in ("y", "dx"):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key


@DIRS
def test_null_outputs_are_skipped_and_two_calls_give_the_same_bits(L, math_mode, up):
    p, m, t, f, b = _case(up, "rand1031", 96, 64)
    full = Run(L, up, m, t).backward(t["dy"])
    again = Run(L, up, m, t).backward(t["dy"])
    for key in ("y", "dx", "dw", "dbias"):
        assert torch.equal(getattr(full, key), getattr(again, key)), key
    for want in (("dx",), ("dw",), ("dbias",), ("dx", "dbias")):
        part = Run(L, up, m, t).backward(t["dy"], want=want)
        for key in ("dx", "dw", "dbias"):
            if key in want:
                assert torch.equal(getattr(part, key), getattr(full, key)), (want, key)
            else:
                assert bool((getattr(part, key) == CANARY).all()), (want, key)
    nobias = Run(L, up, m, t, bias=False)
    assert _err(nobias.y, f - t["b"].double().reshape(1, -1)) < 1e-4


@DIRS
@pytest.mark.parametrize("name", ["rand1031", "clusters_l3"])
def test_autograd_node_against_float64(L, math_mode, name, up):
    from csn_amd import octant_conv_down, octant_conv_up
    c_in, c_out = 64, 96
    p, m, t, f, b = _case(up, name, c_in, c_out)
    x = t["x"].cuda().requires_grad_()
    w = t["w"].cuda().requires_grad_()
    bias = t["b"].cuda().reshape(1, -1).requires_grad_()
    y = (octant_conv_up if up else octant_conv_down)(x, w, bias, m.to("cuda"))
    y.backward(t["dy"].cuda())
    e = _figures({"y": y, "dx": x.grad, "dw": w.grad, "dbias": bias.grad.reshape(-1)}, f, b)
    print(f"[octant] mode {math_mode} autograd {'up' if up else 'down'} {name}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert bias.grad.shape == (1, c_out) and max(e.values()) < 1e-4, e


def test_up_of_down_on_one_map_through_autograd(L, math_mode):
    from csn_amd import octant_conv_down, octant_conv_up
    p, m = _geometry("rand1031")
    m = m.to("cuda")
    t1, t2 = O.tensors(11, p.n_fine, p.n_coarse, 64, 96), O.tensors(12, p.n_coarse, p.n_fine, 96, 32)
    x, w1, w2 = (v.cuda().requires_grad_() for v in (t1["x"], t1["w"], t2["w"]))
    y = octant_conv_up(octant_conv_down(x, w1, None, m), w2, None, m)
    y.backward(t2["dy"].cuda())
    mid = O.down_fwd(p, t1["x"], t1["w"])
    f = O.up_fwd(p, mid, t2["w"])
    b2 = O.up_bwd(p, t2["dy"], mid, t2["w"])
    b1 = O.down_bwd(p, b2["dx"], t1["x"], t1["w"])
    e = {"y": _err(y, f)}
    for k, got, want in (("dx", x.grad, b1["dx"]), ("dw1", w1.grad, b1["dw"]), ("dw2", w2.grad, b2["dw"])):
        e[k] = _err(got, want) / want.abs().max().item()
    print(f"[octant] mode {math_mode} down + up: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e


@pytest.mark.parametrize("widths,c_out", [((256, 128), 128), ((96, 32), 96), ((128, 128), 64)], ids=["256+128", "96+32", "128+128"])
def test_cat_conv3d_is_the_convolution_of_the_concatenation(L, math_mode, widths, c_out):
    from csn_amd import build_kernel_map, cat_conv3d, sparse_conv3d
    pts = R.random_set(300)
    g, _ = R.geometry("s1", pts)
    kmap = build_kernel_map(torch.tensor(pts), 3).to("cuda")
    c_in = sum(widths)
    t = R.tensors(31 + c_in, g.n_in, g.n_out, 27, c_in, c_out)
    f, b = R.fwd(g, t["x"], t["w"]), R.bwd(g, t["dy"], t["x"], t["w"])
    parts = [v.cuda().contiguous().requires_grad_() for v in torch.split(t["x"], list(widths), dim=1)]
    w = t["w"].cuda().requires_grad_()
    y = cat_conv3d(parts, w, kmap)
    y.backward(t["dy"].cuda())
    dx = torch.cat([v.grad for v in parts], dim=1)
    e = {"y": _err(y, f), "dx": _err(dx, b["dx"]) / b["dx"].abs().max().item(), "dw": _err(w.grad, b["dw"]) / b["dw"].abs().max().item()}
    print(f"[octant] mode {math_mode} cat_conv3d {widths}->{c_out}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e
    if c_in <= 256:
        # where the convolution of the concatenation exists, the two agree to the same bound (the sums are ordered differently)
        xc = t["x"].cuda().requires_grad_()
        wc = t["w"].cuda().requires_grad_()
        yc = sparse_conv3d(xc, wc, None, kmap)
        yc.backward(t["dy"].cuda())
        assert (y - yc).abs().max().item() < 1e-4
        assert (dx - xc.grad).abs().max().item() < 1e-4 * b["dx"].abs().max().item()
        assert (w.grad - wc.grad).abs().max().item() < 1e-4 * b["dw"].abs().max().item()
    with pytest.raises(ValueError):
        cat_conv3d(parts[:1], w, kmap)
