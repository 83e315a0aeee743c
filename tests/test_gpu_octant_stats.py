"""GPU parity of the octant products with the BatchNorm statistics epilogue (csn_amd/csrc/octant_conv_stats.hip; include/csn_hip.h
section 26; ``csn_amd.octant_conv_stats``) in math modes 0 and 1: ``z`` bit for bit against section 21's forward without a bias, and
``mean`` / ``invstd`` / the running statistics against float64 (tests/octant_ref.py ``down_fwd`` / ``up_fwd`` and
tests/hrnet_ref.py ``stats``), on the smallest point sets on which the epilogue can go wrong: four empty octants (``even_y``),
segments that end on or one off a 128-entry tile (``box128``, ``box127_129``), random occupancy at 31 / 33 / 129 / 1031 rows, and a
hand-made set whose octants hold 1, 2, 31, 32, 33, 0, 64, 65 fine rows — wave tiles of 0, 1 and 32 rows and short tiles that are not
the last of the grid.  Widths 32 -> 32, 96 -> 64, 64 -> 256, 256 -> 256; the column blocks a wave owns pinned to 1 .. 4
(``CSN_DEV_SCONV_NB``) and left to the launch rule; natural and padded pitches with canaries; two calls bit for bit; a NULL running
pointer; the host refusals with every output still holding its canary; ``octant_conv_stats`` + ``bn_act`` through autograd against
the float64 composition.

Bounds (those tests/test_gpu_hrnet.py holds (15a) to): mean within 1e-4, invstd within 1e-4 max(invstd, invstd^2) (an error dz of
the map moves it by invstd^2 dz), the running statistics within 1e-4; through autograd y within 1e-4 and each gradient within 1e-4
of its tensor's max.

Measured on MI355X, maxima over the cases (fp32 / bf16x3; every test prints its own).  Raw ABI, all point sets and widths, down: mean
2.7e-7 / 1.3e-6, invstd 4.4e-7 / 1.6e-6, running mean 4.8e-8 / 1.3e-7, running variance 9.6e-8 / 3.1e-7; up: mean 6.3e-8 / 1.1e-6,
invstd 1.5e-7 / 1.0e-6, running mean 3.1e-8 / 1.2e-7, running variance 6.2e-8 / 1.1e-7.  Column blocks pinned to 1 .. 4: mean 1.3e-7 /
1.2e-6, invstd 2.0e-7 / 1.4e-6.  Padded pitches: mean 7.7e-8 / 9.4e-7, invstd 2.0e-7 / 1.2e-6.  Through autograd: y 2.8e-6 / 3.2e-5, dx
1.1e-6 / 6.9e-6, dw 1.6e-7 / 5.8e-6, dgamma 2.5e-7 / 5.4e-6, dbeta 4.5e-8 / 4.5e-8.  z equals section 21's forward bit for bit in every case."""
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import octant_ref as O
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
MOM = 0.1


def hand_made():
    """One shape whose octants hold 1, 2, 31, 32, 33, 0, 64, 65 fine rows: coarse cell j (x = 2 j) has a voxel in octant k iff
    j < COUNTS[k].  228 fine rows on 65 coarse rows; the one-weight walk cuts them into tiles of 1, 2, 31, 32, 33, 64, 65 entries:
    waves with 0, 1 and 32 rows, and a short tile in front of full ones."""
    counts = (1, 2, 31, 32, 33, 0, 64, 65)
    return [[0, 2 * j + (k & 1), (k >> 1) & 1, (k >> 2) & 1] for j in range(65) for k in range(8) if j < counts[k]]


SETS = {"even_y": O.even_y, "box128": O.box128, "box127_129": O.box127_129, "hand": hand_made,
        "rand31": lambda: R.random_set(31), "rand33": lambda: R.random_set(33), "rand129": lambda: R.random_set(129),
        "rand1031": lambda: R.random_set(1031)}
WIDTHS = [(32, 32), (96, 64), (64, 256), (256, 256)]
DIRS = pytest.mark.parametrize("up", [False, True], ids=["down", "up"])


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
    L.lib().csn_dev_set(L.DEV_SCONV_NB, 0)


@functools.lru_cache(maxsize=None)
def _geometry(name):
    from csn_amd.minkowski_conv import build_octant_map
    pts = SETS[name]()
    return O.Partition(pts, 1), build_octant_map(torch.tensor(pts), tensor_stride=1)


@functools.lru_cache(maxsize=None)
def _case(up, name, c_in, c_out):
    """Inputs, running statistics and the float64 z and statistics of one case: computed once, shared, never modified."""
    p, m = _geometry(name)
    n_in, n_out = (p.n_coarse, p.n_fine) if up else (p.n_fine, p.n_coarse)
    t = O.tensors(len(name) + c_in + 3 * c_out + int(up), n_in, n_out, c_in, c_out)
    g = torch.Generator().manual_seed(c_out + n_out)
    rm, rv = 0.3 * torch.randn(c_out, generator=g), 0.5 + torch.rand(c_out, generator=g)
    z = (O.up_fwd if up else O.down_fwd)(p, t["x"], t["w"])
    return p, m, t, rm, rv, z, H.stats(z, momentum=MOM, running_mean=rm, running_var=rv)


def _rows(t, pad, fill):
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


def _st():
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One call of section 26 (and, ``plain``, of section 21 on the same inputs) through the raw ABI."""

    def __init__(self, L, up, m, t, rm, rv, pad=0, running=(True, True), ws_short=0, ld_z=None, expect=0):
        lib = L.lib()
        mm = m.to("cuda")
        _, c_in, c_out = t["w"].shape
        n_fine, n_coarse = m.n_fine, m.n_coarse
        n_out = n_fine if up else n_coarse
        self.x, self.xbuf = _rows(t["x"], pad, 1e30)
        self.w = t["w"].cuda().contiguous()
        self.z, self.zbuf = _rows(torch.full((n_out, c_out), CANARY), pad, CANARY)
        self.mean, self.invstd = torch.full((c_out,), CANARY, device="cuda"), torch.full((c_out,), CANARY, device="cuda")
        self.rm = rm.cuda().clone() if running[0] else None
        self.rv = rv.cuda().clone() if running[1] else None
        wb = lib.csn_octant_stats_workspace_bytes(n_fine, n_coarse, c_out, int(up))
        assert wb > 0
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        tail = (_ptr(self.w), _ptr(self.z), (c_out + pad) if ld_z is None else ld_z, _ptr(self.mean), _ptr(self.invstd), _ptr(self.rm),
                _ptr(self.rv), H.EPS, MOM, _ptr(ws), wb - ws_short, _st())
        if up:
            self.status = lib.csn_octant_up_stats_fwd_f32(_ptr(self.x), c_in + pad, n_coarse, _ptr(mm.parent), _ptr(mm.order), _ptr(mm.seg),
                                                          n_fine, c_in, c_out, *tail)
        else:
            self.status = lib.csn_octant_down_stats_fwd_f32(_ptr(self.x), c_in + pad, n_fine, _ptr(mm.children), n_coarse, c_in, c_out, *tail)
        assert self.status == expect, self.status
        self.args = (up, mm, c_in, c_out, n_fine, n_coarse, n_out, pad)

    def plain(self, L):
        """section 21's forward with bias = NULL on the same inputs"""
        up, mm, c_in, c_out, n_fine, n_coarse, n_out, pad = self.args
        lib = L.lib()
        y, _ = _rows(torch.zeros(n_out, c_out), pad, CANARY)
        if up:
            L.check(lib.csn_octant_up_fwd_f32(_ptr(self.x), c_in + pad, n_coarse, _ptr(mm.parent), _ptr(mm.order), _ptr(mm.seg), n_fine,
                                              c_in, c_out, _ptr(self.w), None, _ptr(y), c_out + pad, _st()))
        else:
            L.check(lib.csn_octant_down_fwd_f32(_ptr(self.x), c_in + pad, n_fine, _ptr(mm.children), n_coarse, c_in, c_out, _ptr(self.w),
                                                None, _ptr(y), c_out + pad, _st()))
        return y

    def untouched(self, rm, rv):
        return (bool((self.z == CANARY).all()) and bool((self.mean == CANARY).all()) and bool((self.invstd == CANARY).all())
                and torch.equal(self.rm.cpu(), rm) and torch.equal(self.rv.cpu(), rv))


def _figures(run, ref):
    e = {"mean": (run.mean.cpu().double() - ref["mean"]).abs().max().item(),
         "invstd": ((run.invstd.cpu().double() - ref["invstd"]).abs() / torch.maximum(ref["invstd"], ref["invstd"] ** 2)).max().item()}
    if run.rm is not None:
        e["rmean"] = (run.rm.cpu().double() - ref["running_mean"]).abs().max().item()
    if run.rv is not None:
        e["rvar"] = (run.rv.cpu().double() - ref["running_var"]).abs().max().item()
    return e


def _check(tag, L, run, ref):
    assert torch.equal(run.z, run.plain(L)), tag                                # the bits of section 21
    e = _figures(run, ref)
    print(f"[octant stats] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert torch.isfinite(run.mean).all() and torch.isfinite(run.invstd).all()
    assert max(e.values()) < 1e-4, e
    return e


def test_the_hand_made_set_has_its_segments():
    p = _geometry("hand")[0]
    assert p.segments() == [1, 2, 31, 32, 33, 0, 64, 65] and (p.n_fine, p.n_coarse) == (228, 65)
    assert _geometry("even_y")[0].segments().count(0) == 4
    assert _geometry("box128")[0].segments() == [128] * 8
    assert _geometry("box127_129")[0].segments() == [129, 128, 128, 128, 128, 128, 128, 127]


@DIRS
@pytest.mark.parametrize("c_in,c_out", WIDTHS, ids=[f"{a}to{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("name", list(SETS))
def test_raw_abi_against_float64(L, math_mode, name, c_in, c_out, up):
    p, m, t, rm, rv, _, ref = _case(up, name, c_in, c_out)
    run = Run(L, up, m, t, rm, rv)
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} n {p.n_fine}/{p.n_coarse} {c_in}->{c_out}", L, run, ref)


@DIRS
@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["hand", "box127_129", "rand1031"])
def test_every_instance(L, math_mode, name, nb, up):
    """The column blocks a wave owns pinned to 1 .. 4 at 256 columns (two to eight column groups per row group: the count of a
    tile is written by the first alone)."""
    p, m, t, rm, rv, _, ref = _case(up, name, 64, 256)
    L.lib().csn_dev_set(L.DEV_SCONV_NB, nb)
    try:
        run = Run(L, up, m, t, rm, rv)
        _check(f"mode {math_mode} {'up' if up else 'down'} {name} NB {nb}", L, run, ref)
    finally:
        L.lib().csn_dev_set(L.DEV_SCONV_NB, 0)


@DIRS
@pytest.mark.parametrize("name", ["hand", "rand129"])
def test_padded_pitches_keep_their_canaries(L, math_mode, name, up):
    p, m, t, rm, rv, _, ref = _case(up, name, 96, 64)
    pad = 12
    run = Run(L, up, m, t, rm, rv, pad=pad)
    _check(f"mode {math_mode} {'up' if up else 'down'} {name} pad {pad}", L, run, ref)
    n_out = p.n_fine if up else p.n_coarse
    assert _pad_intact(run.zbuf, n_out, 64, pad, CANARY)


@DIRS
def test_two_calls_give_the_same_bits_and_a_null_running_pointer_leaves_the_other(L, math_mode, up):
    p, m, t, rm, rv, _, ref = _case(up, "rand1031", 64, 256)
    a, b = Run(L, up, m, t, rm, rv), Run(L, up, m, t, rm, rv)
    for k in ("z", "mean", "invstd", "rm", "rv"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for running in ((True, False), (False, True), (False, False)):
        c = Run(L, up, m, t, rm, rv, running=running)
        assert torch.equal(c.mean, a.mean) and torch.equal(c.invstd, a.invstd) and torch.equal(c.z, a.z)
        if running[0]:
            assert torch.equal(c.rm, a.rm)
        if running[1]:
            assert torch.equal(c.rv, a.rv)


@DIRS
def test_host_refusals_leave_every_output_untouched(L, math_mode, up):
    from csn_amd.minkowski_conv import build_octant_map
    p, m, t, rm, rv, _, _ = _case(up, "rand33", 32, 32)
    E_ARG, E_ALIGN, E_WORKSPACE = -1, -2, -6
    # a short workspace, a pitch below the width, a pitch that is no multiple of 4
    assert Run(L, up, m, t, rm, rv, ws_short=16, expect=E_WORKSPACE).untouched(rm, rv)
    assert Run(L, up, m, t, rm, rv, ld_z=28, expect=E_ARG).untouched(rm, rv)
    assert Run(L, up, m, t, rm, rv, ld_z=34, expect=E_ALIGN).untouched(rm, rv)
    # a BatchNorm batch of one row: one voxel gives one coarse row (down); a one-row fine set (up)
    one = build_octant_map(torch.tensor(R.single_voxel()), tensor_stride=1)
    t1 = O.tensors(1, 1, 1, 32, 32)
    assert Run(L, up, one, t1, rm, rv, expect=E_ARG).untouched(rm, rv)


@DIRS
@pytest.mark.parametrize("name,c_in,c_out", [("hand", 96, 64), ("rand1031", 64, 256)])
def test_autograd_node_with_bn_act(L, math_mode, name, c_in, c_out, up):
    """``octant_conv_stats`` + ``bn_act(relu=True)`` against the float64 composition with the GPU's own ReLU mask."""
    import csn_amd
    from csn_amd import functional as CF
    p, m, t, rm, rv, zref, _ = _case(up, name, c_in, c_out)
    g = torch.Generator().manual_seed(7)
    gamma, beta = 1 + 0.2 * torch.randn(c_out, generator=g), 0.3 * torch.randn(c_out, generator=g)
    x = t["x"].cuda().requires_grad_(True)
    w = t["w"].cuda().requires_grad_(True)
    ga, be = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    rm_d, rv_d = rm.cuda().clone(), rv.cuda().clone()
    with CF.math_mode(math_mode):
        z, mean, invstd = csn_amd.octant_conv_stats(x, w, m.to("cuda"), up, rm_d, rv_d, H.EPS, MOM)
        assert not mean.requires_grad and not invstd.requires_grad
        y = csn_amd.bn_act([(z, mean, invstd, ga, be)], None, True, True, H.EPS)
        y.backward(t["dy"].cuda())
    xr, wr = t["x"].double().requires_grad_(True), t["w"].double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = _Ref.apply(p, up, xr, wr)
    mask = (y.detach().cpu() > 0)
    yr, pre = H.bn_act([{"z": zr, "gamma": gr, "beta": br}], None, True, True, mask=mask)
    yr.backward(t["dy"].double())
    near = pre.detach().abs() < 1e-4
    e = {"y": ((y.detach().cpu().double() - yr.detach()).abs() * ~near).max().item()}
    for k, got, want in (("dx", x.grad, xr.grad), ("dw", w.grad, wr.grad), ("dgamma", ga.grad, gr.grad), ("dbeta", be.grad, br.grad)):
        e[k] = (got.cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
    print(f"[octant stats] autograd mode {math_mode} {'up' if up else 'down'} {name}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert near.float().mean().item() <= 1e-3
    assert max(e.values()) < 1e-4, e
    s = H.stats(zref, momentum=MOM, running_mean=rm, running_var=rv)
    assert (rm_d.cpu().double() - s["running_mean"]).abs().max() < 1e-4 and (rv_d.cpu().double() - s["running_var"]).abs().max() < 1e-4
    # needs_input_grad is honoured: a constant weight gets no gradient and the node still runs
    x2 = t["x"].cuda().requires_grad_(True)
    with CF.math_mode(math_mode):
        z2, _, _ = csn_amd.octant_conv_stats(x2, t["w"].cuda(), m.to("cuda"), up, None, None, H.EPS, MOM)
        z2.backward(torch.ones_like(z2))
    assert x2.grad is not None and torch.equal(z2.detach(), z.detach())


class _Ref(torch.autograd.Function):
    """tests/octant_ref.py's forward and backward as a float64 autograd node."""

    @staticmethod
    def forward(ctx, p, up, x, w):
        ctx.p, ctx.up = p, up
        ctx.save_for_backward(x, w)
        return (O.up_fwd if up else O.down_fwd)(p, x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        b = (O.up_bwd if ctx.up else O.down_bwd)(ctx.p, dy, x, w)
        return None, None, b["dx"], b["dw"]


def test_cpu_tensors_and_one_row_batches_are_refused(L):
    import csn_amd
    from csn_amd._lib import CsnError
    from csn_amd.minkowski_conv import build_octant_map
    m = build_octant_map(torch.tensor(R.random_set(33)), tensor_stride=1)
    with pytest.raises(CsnError):
        csn_amd.octant_conv_stats(torch.zeros(m.n_fine, 32), torch.zeros(8, 32, 32), m, False, None, None, 1e-5, 0.1)
    one = build_octant_map(torch.tensor(R.single_voxel()), tensor_stride=1).to("cuda")
    for up in (False, True):
        with pytest.raises(ValueError, match="more than 1 value"):
            csn_amd.octant_conv_stats(torch.zeros(1, 32, device="cuda"), torch.zeros(8, 32, 32, device="cuda"), one, up, None, None, 1e-5, 0.1)
