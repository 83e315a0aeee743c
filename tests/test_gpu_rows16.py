"""GPU parity of the single-product row products — math modes "bf16" (forward + backward) and "fp16" (forward) with
``csn_set_thread_rows16(1)`` in include/csn_hip.h sections 13 (fc_layer), 14 (sparse convolution) and 15a (its statistics form);
csn_amd/csrc/rows_mma.h, sparse_conv.hip, rows_fc.hip — through the raw ABI, and of the Python switch ``tuning.rows_single_product``.

Yardstick: the float64 references (tests/sparse_conv_ref.py, tests/rows_fc_ref.py) fed operands rounded on the CPU to the mode's type
(tests/rows16_ref.py): x and w for a forward; dy, x and w as bf16 for the gradient products dx and dw.  The bias stays fp32, and
dbias, dgamma and dbeta are no matrix products: they are sums of fp32 values and are held against the unrounded ones.  The product of
two bf16 or two fp16 values is exact in fp32, so what remains is fp32 accumulation in the instruction bf16x3 uses: the bounds are the
project's contract — y within 1e-4 absolute, each gradient within 1e-4 of its tensor's maximum.  That the single product really ran
shows against a second yardstick, the same reference on UNROUNDED operands: y is at most a quarter as far from the rounded reference
as the two references are apart.  fp16 cases zero every operand entry below 2^-14 in magnitude on both sides (asserted): nothing hinges on
how the matrix instruction treats subnormals.  In fc_layer dx and dw are held against float64 products of the GPU's OWN dz rounded to
bf16 (dz is no matrix product; it is read back through an exact-fp32 call on an identity weight): a float64 dz rounded on its own
can fall on the other side of a rounding boundary, which is not the kernels' error.

The whole network (``HRNetBackbone`` 2S, training, 300 voxels, switch on) has no derivable bound — rounding decisions flip between an
fp32 and a float64 activation and travel through 30-odd BatchNorms — so its yardstick is the reference alone: E_ref is the error of
the rounded restatement (``rows16_ref.conv``, the GPU's ReLU masks) against the exact float64 one under the same masks, per compared
tensor, and the GPU may err by max(1e-4, 2 E_ref): two draws of the same rounding noise, the margin between ``fused=True`` and
``fused=False`` in tests/test_gpu_hrnet.py.

Measured on MI355X, maxima over the cases (bf16 / fp16; every test prints its own).  Convolution at stride 1: y 2.8e-6 / 4.0e-6, dx
9.2e-7, dw 1.2e-7, dbias 5.0e-8, the two references 5.9e-4 ... 7.6e-3 / 9.2e-5 ... 1.2e-3 apart in y.  Every instance pinned on 1031
rows: y 1.7e-6 / 1.4e-6, dx 7.4e-7, dw 1.6e-7.  Stride 2 and transposed: y 7.8e-7 / 7.5e-7, dx 3.0e-7, dw 9.1e-8.  Padded pitches: y 9.1e-8
/ 1.5e-7, the bits of the natural pitch.  Statistics epilogue: z 1.6e-6 / 1.3e-6, mean 1.8e-8, invstd 3.8e-8, running statistics <=
6.1e-8.  fc_layer: y 2.0e-6 / 1.7e-6, z 1.8e-6 / 1.6e-6, mean 8.5e-8, running statistics <= 6.6e-8, references 4.1e-4 ... 1.4e-2 / 1.3e-4
... 1.7e-3 apart; bf16 backward dx 2.3e-7, dw 1.5e-7, dbias 2.4e-7, dgamma 5.6e-7, dbeta 5.1e-8.  Backbone 2S, training, 300 voxels,
GPU (E_ref): bf16 y 1.6e-1 (1.4e-1), gradients 1.2e-2 (1.2e-2), running statistics 6.5e-5 (7.7e-5), largest GPU / E_ref of a tensor
1.33; fp16 y 1.7e-2 (1.5e-2), gradients 7.6e-3 (6.9e-3), running statistics 1.1e-5 (1.3e-5), largest ratio 1.39."""
import contextlib
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import rows16_ref as R16
from tests import rows_fc_ref as FC
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
EPS, MOM = 1e-5, 0.02
KINDS = ["bf16", "fp16"]
SETS = {"single": R.single_voxel, "rand31": lambda: R.random_set(31), "rand33": lambda: R.random_set(33),
        "rand129": lambda: R.random_set(129), "rand1031": lambda: R.random_set(1031), "clusters": R.two_clusters}
WIDTHS = [(32, 32, 3), (32, 64, 3), (64, 64, 3), (256, 256, 3), (32, 32, 5)]
# (c_in, c_out, column blocks per wave), as tests/test_gpu_sparse_conv.py: one and two column groups, a last group with 1, 2 or 3
# blocks past the width; c_in = 64, 96, 128 take the weight gradient's TA 2, 3, 4 (c_in = 32 and TA 1: WIDTHS)
NB_CASES = [(64, 64, 2), (96, 96, 3), (128, 128, 4), (160, 160, 3), (160, 96, 4), (192, 224, 3), (256, 256, 4), (224, 192, 4)]
FC_CASES = [(2, 32, 32), (31, 480, 256), (65, 992, 256), (129, 480, 128), (257, 416, 64)]


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@contextlib.contextmanager
def arith(L, mode, flag=1):
    """The calling thread's library calls in math mode ``mode`` (0..3, or "bf16" / "fp16") with the rows16 flag at ``flag``."""
    lib = L.lib()
    L.check(lib.csn_set_thread_math_mode(R16.MODES.get(mode, mode)))
    L.check(lib.csn_set_thread_rows16(flag))
    try:
        yield
    finally:
        lib.csn_set_thread_rows16(0)
        lib.csn_set_thread_math_mode(-1)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


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


def _operands(t, kind, keys):
    """The case's tensors as the kernels of ``kind`` get them: fp16 operands hold no subnormal (asserted)."""
    if kind != "fp16":
        return t
    t = {**t, **{k: R16.no_subnormals(t[k]) for k in keys}}
    for k in keys:
        assert not bool(((t[k] != 0) & (t[k].abs() < R16.FP16_MIN_NORMAL)).any()), k
    return t


# ------------------------------------------------------------------------------------------------------
# sparse convolution (14)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geometry(mode, name, k):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = SETS[name]()
    if mode == "s1":
        return R.geometry("s1", pts, k=k)[0], build_kernel_map(torch.tensor(pts), kernel_size=k)
    down = build_kernel_map(torch.tensor(pts), kernel_size=3, stride=2)
    if mode == "s2":
        return R.geometry("s2", pts)[0], down
    return R.geometry("tr", R.down_coords([tuple(c) for c in pts], 1), fine=pts)[0], down.transpose()


@functools.lru_cache(maxsize=None)
def _case(mode, name, c_in, c_out, k, kind):
    """Geometry, map, inputs, and the float64 forward on rounded and on unrounded operands; shared, never modified."""
    g, m = _geometry(mode, name, k)
    t = _operands(R.tensors(len(name) + c_in + 3 * c_out + k, g.n_in, g.n_out, g.KV, c_in, c_out), kind, ("x", "w"))
    return g, m, t, R.fwd(g, R16.round16(t["x"], kind), R16.round16(t["w"], kind), t["b"]), R.fwd(g, t["x"], t["w"], t["b"])


@functools.lru_cache(maxsize=None)
def _grads(mode, name, c_in, c_out, k):
    """The float64 gradient products on bf16-rounded dy, x and w; dbias is the sum of the fp32 dy."""
    g, _, t, _, _ = _case(mode, name, c_in, c_out, k, "bf16")
    b = R.bwd(g, R16.round16(t["dy"], "bf16"), R16.round16(t["x"], "bf16"), R16.round16(t["w"], "bf16"))
    b["dbias"] = t["dy"].double().sum(0)
    return b


class Conv:
    """One forward (+ backward) of section 14 through the raw ABI in math mode ``mode`` with the rows16 flag at ``flag``."""

    def __init__(self, L, m, t, mode, flag=1, pad=0, bias=True):
        lib = L.lib()
        self.L, self.m, self.pad, self.flag = L, m.to("cuda"), pad, flag
        self.KV, self.c_in, self.c_out = t["w"].shape
        self.n_in, self.n_out = m.n_in, m.n_out
        self.x, self.xbuf = _rows(t["x"], pad, 1e30)
        self.w = t["w"].cuda().contiguous()
        self.b = t["b"].cuda().contiguous() if bias else None
        self.y, self.ybuf = _rows(torch.zeros(self.n_out, self.c_out), pad, CANARY)
        if not pad:
            self.y.fill_(CANARY)
        with arith(L, mode, flag):
            L.check(lib.csn_sparse_conv_fwd_f32(_ptr(self.x), self.c_in + pad, self.n_in, _ptr(self.m.fwd), self.n_out, self.KV, self.c_in,
                                                self.c_out, _ptr(self.w), _ptr(self.b), _ptr(self.y), self.c_out + pad, _st()), "fwd")

    def backward(self, dy_cpu, mode="bf16", expect=0):
        lib, pad = self.L.lib(), self.pad
        self.dy, self.dybuf = _rows(dy_cpu, pad, 1e30)
        self.dx, self.dxbuf = _rows(torch.zeros(self.n_in, self.c_in), pad, CANARY)
        if not pad:
            self.dx.fill_(CANARY)
        self.dw = torch.full((self.KV, self.c_in, self.c_out), CANARY, device="cuda")
        self.dbias = torch.full((self.c_out,), CANARY, device="cuda")
        wb = lib.csn_sparse_conv_workspace_bytes(self.n_in, self.n_out, self.KV, self.c_in, self.c_out, 1)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        with arith(self.L, mode, self.flag):
            rc = lib.csn_sparse_conv_bwd_f32(_ptr(self.dy), self.c_out + pad, _ptr(self.x), self.c_in + pad, self.n_in, self.n_out, self.KV,
                                             self.c_in, self.c_out, _ptr(self.m.fwd), _ptr(self.m.bwd_table), _ptr(self.w), _ptr(self.dx),
                                             self.c_in + pad, _ptr(self.dw), _ptr(self.dbias), _ptr(ws), wb, _st())
        assert rc == expect, rc
        return self


def _check_conv(tag, run, f, f_exact, b=None):
    """y within 1e-4 of the rounded reference and at most a quarter as far from it as the unrounded reference is; every gradient
    within 1e-4 of its tensor's max.  Prints the figures."""
    e = {"y": _err(run.y, f)}
    apart = (f - f_exact).abs().max().item()
    for k in ("dx", "dw", "dbias") if b is not None else ():
        e[k] = _err(getattr(run, k), b[k]) / max(b[k].abs().max().item(), 1e-30)
        assert torch.isfinite(getattr(run, k)).all(), k
    print(f"[rows16] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" | references apart {apart:.1e}")
    assert torch.isfinite(run.y).all()
    assert max(e.values()) < 1e-4, e
    assert e["y"] <= 0.25 * apart, (e["y"], apart)
    return e


def _conv_case(L, tag, mode, name, c_in, c_out, k, kind, pad=0):
    g, m, t, f, f_exact = _case(mode, name, c_in, c_out, k, kind)
    run = Conv(L, m, t, kind, pad=pad)
    if kind == "bf16":
        run.backward(t["dy"])
    _check_conv(f"{kind} {tag} {name} rows {g.n_in}->{g.n_out} {c_in}->{c_out} k{k}", run, f, f_exact,
                _grads(mode, name, c_in, c_out, k) if kind == "bf16" else None)
    return run


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c_in,c_out,k", WIDTHS, ids=[f"{a}to{b}k{k}" for a, b, k in WIDTHS])
@pytest.mark.parametrize("name", list(SETS))
def test_stride_1_against_float64_on_rounded_operands(L, name, c_in, c_out, k, kind):
    """Either side of the 32-row wave tile and the 128-row work-group tile, tiles that skip every offset but the centre (clusters),
    several split-K chunks of the weight gradient (1031 rows)."""
    _conv_case(L, "s1", "s1", name, c_in, c_out, k, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c_in,c_out,nb", NB_CASES, ids=[f"{a}to{b}nb{n}" for a, b, n in NB_CASES])
def test_every_instance_against_float64(L, c_in, c_out, nb, kind):
    """CSN_DEV_SCONV_NB pins the column blocks a wave owns, so 1031 rows reach every instance of the forward and of dx; the pinned
    launches give the bits of the launch rule's own choice."""
    g, m, t, f, f_exact = _case("s1", "rand1031", c_in, c_out, 3, kind)
    lib = L.lib()
    assert lib.csn_dev_get(L.DEV_SCONV_NB) == 0
    plain = Conv(L, m, t, kind)
    assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) == 0
    try:
        run = Conv(L, m, t, kind)
        if kind == "bf16":
            plain.backward(t["dy"])
            run.backward(t["dy"])
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    _check_conv(f"{kind} nb {nb} n {g.n_in} {c_in}->{c_out}", run, f, f_exact, _grads("s1", "rand1031", c_in, c_out, 3) if kind == "bf16" else None)
    for key in ("y", "dx") if kind == "bf16" else ("y",):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c_in,c_out", [(64, 128), (128, 64)], ids=["64to128", "128to64"])
@pytest.mark.parametrize("name", ["rand129", "rand1031"])
@pytest.mark.parametrize("mode", ["s2", "tr"])
def test_stride_2_and_transposed(L, mode, name, c_in, c_out, kind):
    """One map and its ``transpose()``."""
    g, m, _, _, _ = _case(mode, name, c_in, c_out, 3, kind)
    assert m.transposed == (mode == "tr") and (g.n_in, g.n_out) == (m.n_in, m.n_out) and g.n_in != g.n_out
    _conv_case(L, mode, mode, name, c_in, c_out, 3, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["rand33", "rand129"])
def test_padded_pitches_leave_the_canary_and_the_bits(L, name, kind):
    """4 floats of padding per row and a base 16 bytes into the buffer."""
    g, m, t, _, _ = _case("s1", name, 32, 32, 3, kind)
    run = _conv_case(L, "padded", "s1", name, 32, 32, 3, kind, pad=4)
    plain = _conv_case(L, "natural", "s1", name, 32, 32, 3, kind)
    assert _pad_intact(run.ybuf, g.n_out, 32, 4, CANARY) and _pad_intact(run.xbuf, g.n_in, 32, 4, 1e30)
    if kind == "bf16":
        assert _pad_intact(run.dxbuf, g.n_in, 32, 4, CANARY) and _pad_intact(run.dybuf, g.n_out, 32, 4, 1e30)
    for key in ("y", "dx", "dw", "dbias") if kind == "bf16" else ("y",):
        assert torch.equal(getattr(run, key), getattr(plain, key)), key


# ------------------------------------------------------------------------------------------------------
# the statistics epilogue (15a)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("name", ["rand31", "rand129", "rand1031"])
def test_statistics_epilogue(L, name, c, kind):
    """z bit-equal to csn_sparse_conv_fwd_f32 in the same mode; mean, invstd and the running statistics against the float64
    statistics of the rounded-operand z, with the bounds of tests/test_gpu_hrnet.py::test_conv_stats_forward (1e-4 absolute;
    invstd: 1e-4 max(invstd, invstd^2))."""
    g, m, t, _, _ = _case("s1", name, c, c, 3, kind)
    z64 = R.fwd(g, R16.round16(t["x"], kind), R16.round16(t["w"], kind))
    gen = torch.Generator().manual_seed(c)
    rm, rv = 0.1 * torch.randn(c, generator=gen), 1 + 0.1 * torch.randn(c, generator=gen).abs()
    ref = H.stats(z64, H.EPS, 0.1, rm, rv)
    lib = L.lib()
    plain = Conv(L, m, t, kind, bias=False)
    md = m.to("cuda")
    x, w = t["x"].cuda().contiguous(), t["w"].cuda().contiguous()
    z = torch.full((g.n_out, c), CANARY, device="cuda")
    mean, invstd = torch.full((c,), CANARY, device="cuda"), torch.full((c,), CANARY, device="cuda")
    rm_d, rv_d = rm.cuda(), rv.cuda()
    wb = lib.csn_sparse_conv_stats_workspace_bytes(g.n_out, c)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    with arith(L, kind):
        L.check(lib.csn_sparse_conv_stats_fwd_f32(_ptr(x), c, g.n_in, _ptr(md.fwd), g.n_out, 27, c, c, _ptr(w), _ptr(z), c, _ptr(mean),
                                                  _ptr(invstd), _ptr(rm_d), _ptr(rv_d), H.EPS, 0.1, _ptr(ws), wb, _st()), "stats fwd")
    assert torch.equal(z, plain.y), "z differs from csn_sparse_conv_fwd_f32"
    e = {"z": _err(z, z64), "mean": _err(mean, ref["mean"]),
         "invstd": ((invstd.cpu().double() - ref["invstd"]).abs() / torch.maximum(ref["invstd"], ref["invstd"] ** 2)).max().item(),
         "rmean": _err(rm_d, ref["running_mean"]), "rvar": _err(rv_d, ref["running_var"])}
    print(f"[rows16] {kind} conv_stats {name} {c}->{c}: " + " ".join(f"{q} {v:.1e}" for q, v in e.items()))
    assert all(v < 1e-4 for v in e.values()), e


# ------------------------------------------------------------------------------------------------------
# fc_layer (13)
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fc_case(n, c_in, c_out, kind):
    """Inputs and the float64 forwards (training / eval) on rounded operands; shared, never modified."""
    i = _operands(FC.inputs(1000 + n + c_in + c_out, n, c_in, c_out), kind, ("x", "w"))
    f = {tr: FC.fwd(R16.round16(i["x"], kind), R16.round16(i["w"], kind), i["b"], i["gamma"], i["beta"], i["running_mean"],
                    i["running_var"], EPS, MOM, tr) for tr in (True, False)}
    return i, f


class Fc:
    """One forward (+ backward) of section 13 through the raw ABI."""

    def __init__(self, L, i, training, mode, flag=1):
        lib = L.lib()
        self.L, self.i, self.training, self.flag = L, i, training, flag
        self.n, self.c_in = i["x"].shape
        self.c_out = i["w"].shape[0]
        n, c_in, c_out = self.n, self.c_in, self.c_out
        d = lambda k: i[k].cuda().contiguous()
        self.x, self.w, self.b, self.gamma, self.beta = d("x"), d("w"), d("b"), d("gamma"), d("beta")
        self.rm, self.rv = d("running_mean").clone(), d("running_var").clone()
        self.y = torch.full((n, c_out), CANARY, device="cuda")
        self.z = torch.full((n, c_out), CANARY, device="cuda")
        self.mean, self.invstd = torch.empty(c_out, device="cuda"), torch.empty(c_out, device="cuda")
        wb = lib.csn_rows_fc_workspace_bytes(n, c_in, c_out, int(training), 0)
        ws = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        with arith(L, mode, flag):
            L.check(lib.csn_rows_fc_fwd_f32(_ptr(self.x), c_in, n, c_in, c_out, _ptr(self.w), _ptr(self.b), _ptr(self.gamma), _ptr(self.beta),
                                            _ptr(self.rm), _ptr(self.rv), EPS, MOM, int(training), _ptr(self.y), c_out,
                                            _ptr(self.z) if training else None, c_out, _ptr(self.mean) if training else None,
                                            _ptr(self.invstd) if training else None, _ptr(ws) if training else None, wb, _st()), "fwd")

    def _bwd(self, x, c_in, w, dx, dw, dbias, mode, flag):
        lib, n, c_out = self.L.lib(), self.n, self.c_out
        wb = lib.csn_rows_fc_workspace_bytes(n, c_in, c_out, int(self.training), 1)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        sm, ss = (self.mean, self.invstd) if self.training else (self.rm, self.rv)
        with arith(self.L, mode, flag):
            return lib.csn_rows_fc_bwd_f32(_ptr(self.dy), c_out, _ptr(self.y), c_out, _ptr(self.z) if self.training else None, c_out, _ptr(x),
                                           c_in, n, c_in, c_out, _ptr(w), _ptr(self.b), _ptr(self.gamma), _ptr(sm), _ptr(ss), EPS,
                                           int(self.training), _ptr(dx), c_in, _ptr(dw), _ptr(dbias), _ptr(self.dgamma), _ptr(self.dbeta),
                                           _ptr(ws), wb, _st())

    def backward(self, dy_cpu, mode="bf16", expect=0):
        n, c_in, c_out = self.n, self.c_in, self.c_out
        self.dy = dy_cpu.cuda().contiguous()
        self.dx = torch.full((n, c_in), CANARY, device="cuda")
        self.dw = torch.full((c_out, c_in), CANARY, device="cuda")
        self.dbias = torch.full((c_out,), CANARY, device="cuda")
        self.dgamma, self.dbeta = torch.full((c_out,), CANARY, device="cuda"), torch.full((c_out,), CANARY, device="cuda")
        assert self._bwd(self.x, c_in, self.w, self.dx, self.dw, self.dbias, mode, self.flag) == expect
        return self

    def own_dz(self):
        """The dz of this run's backward, an elementwise fp32 expression of dy, y, z and the statistics that no math mode touches:
        dx of an exact-fp32 call (mode 0) on the identity weight is dz itself."""
        c = self.c_out
        eye, zeros, dz = torch.eye(c, device="cuda"), torch.zeros(self.n, c, device="cuda"), torch.full((self.n, c), CANARY, device="cuda")
        keep = self.dgamma.clone(), self.dbeta.clone()
        assert self._bwd(zeros, c, eye, dz, None, None, 0, 0) == 0
        self.dgamma, self.dbeta = keep
        return dz.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,c_in,c_out", FC_CASES, ids=[f"{a}x{b}x{c}" for a, b, c in FC_CASES])
def test_fc_layer_against_float64_on_rounded_operands(L, n, c_in, c_out, kind):
    """Training and eval forward (the folded epilogue) in both modes, the ReLU mask, and the bf16 backward under the GPU's mask."""
    i, fs = _fc_case(n, c_in, c_out, kind)
    for training in (True, False):
        f = fs[training]
        run = Fc(L, i, training, kind)
        tag = f"{kind} fc {n}x{c_in}x{c_out} {'train' if training else 'eval'}"
        e = {"y": _err(run.y, f["y"])}
        if training:
            e.update(mean=_err(run.mean, f["mean"]), rm=_err(run.rm, f["running_mean"]), rv=_err(run.rv, f["running_var"]), z=_err(run.z, f["z"]))
        else:
            assert torch.equal(run.rm.cpu(), i["running_mean"]) and torch.equal(run.rv.cpu(), i["running_var"])
            assert bool((run.z == CANARY).all())                                  # eval writes nothing but y
        exact = FC.fwd(i["x"], i["w"], i["b"], i["gamma"], i["beta"], i["running_mean"], i["running_var"], EPS, MOM, training)
        apart = (f["y"] - exact["y"]).abs().max().item()
        decided = f["a"].abs() >= 1e-4
        undecided = 1.0 - decided.double().mean().item()
        print(f"[rows16] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" undecided {undecided:.2e} | references apart {apart:.1e}")
        assert max(e.values()) < 1e-4, e
        assert e["y"] <= 0.25 * apart, (e["y"], apart)
        assert undecided <= 1e-3
        assert torch.equal((run.y.cpu() > 0)[decided], (f["a"] > 0)[decided])
        if kind != "bf16":
            continue
        run.backward(i["dy"])
        b = FC.bwd(i["dy"], run.y.cpu() > 0, R16.round16(i["x"], "bf16"), R16.round16(i["w"], "bf16"), i["gamma"], f, training)
        dz = R16.round16(run.own_dz(), "bf16").double()
        b["dx"], b["dw"] = dz @ R16.round16(i["w"], "bf16").double(), dz.t() @ R16.round16(i["x"], "bf16").double()
        small = n < 31
        scale = {"dx": b["scale_dx"] if small else b["dx"].abs().max(), "dw": b["scale_dw"] if small else b["dw"].abs().max(),
                 "dbias": b["scale_dbias"] if (small or training) else b["dbias"].abs().max(),
                 "dgamma": b["dgamma"].abs().max(), "dbeta": b["dbeta"].abs().max()}
        got = {"dx": run.dx, "dw": run.dw, "dbias": run.dbias, "dgamma": run.dgamma, "dbeta": run.dbeta}
        eb = {k: _err(got[k], b[k]) / max(float(scale[k]), 1e-30) for k in got}
        print(f"[rows16] {tag} backward: " + " ".join(f"{k} {v:.1e}" for k, v in eb.items()))
        for k, v in got.items():
            assert torch.isfinite(v).all(), k
        assert max(eb.values()) < 1e-4, eb


# ------------------------------------------------------------------------------------------------------
# the flag
# ------------------------------------------------------------------------------------------------------
CONV_OUT, FC_OUT = ("y", "dx", "dw", "dbias"), ("y", "z", "mean", "invstd", "rm", "rv", "dx", "dw", "dbias", "dgamma", "dbeta")


def _same(a, b, keys):
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_flag_semantics(L):
    g, m, t, _, _ = _case("s1", "rand1031", 64, 64, 3, "bf16")
    i, _ = _fc_case(129, 480, 128, "bf16")
    conv = lambda mode, flag, bmode=None: Conv(L, m, t, mode, flag).backward(t["dy"], mode if bmode is None else bmode)
    fc = lambda mode, flag, bmode=None: Fc(L, i, True, mode, flag).backward(i["dy"], mode if bmode is None else bmode)
    x3 = conv(1, 0), fc(1, 0)
    _same(conv(1, 1), x3[0], CONV_OUT)                                  # modes 0 and 1 do not see the flag
    _same(fc(1, 1), x3[1], FC_OUT)
    _same(conv(0, 1), conv(0, 0), CONV_OUT)
    _same(fc(0, 1), fc(0, 0), FC_OUT)
    _same(conv(2, 0), x3[0], CONV_OUT)                                  # flag 0: modes 2 / 3 run as mode 1
    _same(fc(2, 0), x3[1], FC_OUT)
    _same(conv(3, 0, 2), x3[0], CONV_OUT)
    one = conv(2, 1), fc(2, 1)
    assert not torch.equal(one[0].y, x3[0].y) and not torch.equal(one[1].y, x3[1].y)
    _same(conv(2, 1), one[0], CONV_OUT)                                 # two identical calls give the same bits
    _same(fc(2, 1), one[1], FC_OUT)
    # flag 1, mode 3: the backward entry points refuse before any launch
    c3 = Conv(L, m, t, 3, 1).backward(t["dy"], 3, expect=-1)
    f3 = Fc(L, i, True, 3, 1).backward(i["dy"], 3, expect=-1)
    torch.cuda.synchronize()
    for run, keys in ((c3, ("dx", "dw", "dbias")), (f3, ("dx", "dw", "dbias", "dgamma", "dbeta"))):
        for k in keys:
            assert bool((getattr(run, k) == CANARY).all()), k
    assert not torch.equal(c3.y, one[0].y) and not torch.equal(c3.y, x3[0].y)          # the fp16 forward is a product of its own
    assert L.lib().csn_get_thread_rows16() == 0


# ------------------------------------------------------------------------------------------------------
# the Python switch
# ------------------------------------------------------------------------------------------------------
def _module_conv(t, m, mode, switch):
    from csn_amd import functional as CF
    from csn_amd import sparse_conv3d, tuning
    x, w, b = (t[k].cuda().requires_grad_(True) for k in ("x", "w", "b"))
    with CF.math_mode(mode), tuning.override(rows_single_product=switch):
        y = sparse_conv3d(x, w, b, m.to("cuda"))
    y.backward(t["dy"].cuda())                                            # outside the blocks: the node kept mode and switch
    return y.detach(), x.grad, w.grad, b.grad


def _module_fc(i, mode, switch):
    from csn_amd import functional as CF
    from csn_amd import tuning
    from csn_amd.minkowski_csn import BackboneFC
    c_out, c_in = i["w"].shape
    mod = BackboneFC(c_in, c_out, bn_momentum=MOM, eps=EPS)
    with torch.no_grad():
        mod[0].weight.copy_(i["w"]); mod[0].bias.copy_(i["b"]); mod[1].weight.copy_(i["gamma"]); mod[1].bias.copy_(i["beta"])
        mod[1].running_mean.copy_(i["running_mean"]); mod[1].running_var.copy_(i["running_var"])
    mod = mod.cuda().train()
    x = i["x"].cuda().requires_grad_(True)
    with CF.math_mode(mode), tuning.override(rows_single_product=switch):
        y = mod(x)
    y.backward(i["dy"].cuda())
    return y.detach(), x.grad, mod[0].weight.grad, mod[0].bias.grad, mod[1].weight.grad, mod[1].bias.grad


@pytest.mark.parametrize("kind", KINDS)
def test_python_switch_reaches_the_kernels(L, kind):
    """Switch on: autograd gives the bits of the raw ABI with the flag (an fp16 forward runs its backward in bf16); switch off:
    the bits of math_mode("bf16x3")."""
    g, m, t, _, _ = _case("s1", "rand1031", 64, 64, 3, kind)
    raw = Conv(L, m, t, kind).backward(t["dy"], "bf16")
    for got, want in zip(_module_conv(t, m, kind, True), (raw.y, raw.dx, raw.dw, raw.dbias)):
        assert torch.equal(got, want)
    for got, want in zip(_module_conv(t, m, kind, False), _module_conv(t, m, "bf16x3", False)):
        assert torch.equal(got, want)
    i, _ = _fc_case(129, 480, 128, kind)
    raw = Fc(L, i, True, kind).backward(i["dy"], "bf16")
    for got, want in zip(_module_fc(i, kind, True), (raw.y, raw.dx, raw.dw, raw.dbias, raw.dgamma, raw.dbeta)):
        assert torch.equal(got, want)
    for got, want in zip(_module_fc(i, kind, False), _module_fc(i, "bf16x3", False)):
        assert torch.equal(got, want)
    assert L.lib().csn_get_thread_rows16() == 0


# ------------------------------------------------------------------------------------------------------
# the whole network
# ------------------------------------------------------------------------------------------------------
def _net_reference(pyr, feats, dy, params, S, masks, conv_fn):
    p = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in params.items()}
    f64 = feats.double().requires_grad_(True)
    rows, _, new = H.backbone(pyr, f64, p, S, True, masks=masks, conv_fn=conv_fn)
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    grads = torch.autograd.grad(rows, [f64] + [p[k] for k in names], dy.double())
    return rows.detach(), dict(zip(["feats"] + names, grads)), new


def _net_errors(rows, grads, running, exact):
    """Per compared tensor, against the exact reference: y absolute, each gradient relative to its tensor's max, the running
    statistics absolute."""
    rows_e, grads_e, new_e = exact
    e = {"y": (rows.double() - rows_e).abs().max().item()}
    for k, w in grads_e.items():
        e["d " + k] = (grads[k].double() - w).abs().max().item() / max(w.abs().max().item(), 1e-300)
    for k, (rm, rv) in new_e.items():
        e["rm " + k] = (running[k][0].double() - rm).abs().max().item()
        e["rv " + k] = (running[k][1].double() - rv).abs().max().item()
    return e


@pytest.mark.parametrize("kind", KINDS)
def test_backbone_2s_against_the_rounded_restatement(L, kind):
    """(module docstring) The GPU's error against exact float64 under its own ReLU masks is at most max(1e-4, 2 E_ref) per tensor."""
    from csn_amd import HRNetBackbone, build_pyramid, tuning
    from csn_amd import functional as CF
    S, ff = 2, 4
    pts = R.random_set(300)
    gen = torch.Generator().manual_seed(len(pts))
    feats, dy = torch.randn(len(pts), 3, generator=gen), torch.randn(len(pts), 32 + 32 * ff * (2 ** S - 1), generator=gen)
    params = H.params(S, ff)
    if kind == "fp16":
        feats = R16.no_subnormals(feats)
        params = {k: (R16.no_subnormals(v) if v.is_floating_point() else v) for k, v in params.items()}
    bb = HRNetBackbone(3, S, ff, fused=True).cuda().train()
    bb.load_state_dict(params)
    x = feats.cuda().requires_grad_(True)
    trace = {}
    with CF.math_mode(kind), tuning.override(rows_single_product=True):
        rows = bb(x, build_pyramid(torch.tensor(pts), S).to("cuda"), trace)
        rows.backward(dy.cuda())
    masks = {k: v.cpu() > 0 for k, v in trace.items()}
    pyr = H.Pyramid(pts, S)
    exact = _net_reference(pyr, feats, dy, params, S, masks, H.conv)
    rounded = _net_reference(pyr, feats, dy, params, S, masks, R16.conv(kind))
    sd = bb.state_dict()
    got = _net_errors(rows.detach().cpu(), {"feats": x.grad.cpu(), **{k: v.grad.cpu() for k, v in bb.named_parameters()}},
                      {k: (sd[k + ".running_mean"].cpu(), sd[k + ".running_var"].cpu()) for k in exact[2]}, exact)
    e_ref = _net_errors(rounded[0], rounded[1], rounded[2], exact)
    assert sorted(got) == sorted(e_ref)
    worst = lambda e, pre: max(v for k, v in e.items() if k.startswith(pre))
    print(f"[rows16] {kind} backbone 2S train: GPU y {got['y']:.1e} gradients {worst(got, 'd '):.1e} running {max(worst(got, 'rm '), worst(got, 'rv ')):.1e}"
          f" | E_ref y {e_ref['y']:.1e} gradients {worst(e_ref, 'd '):.1e} running {max(worst(e_ref, 'rm '), worst(e_ref, 'rv ')):.1e}"
          f" | largest GPU / E_ref {max(got[k] / max(e_ref[k], 1e-300) for k in got if got[k] > 1e-4):.2f}" if any(v > 1e-4 for v in got.values())
          else f"[rows16] {kind} backbone 2S train: every GPU error below 1e-4")
    bad = {k: (got[k], e_ref[k]) for k in got if got[k] > max(1e-4, 2 * e_ref[k])}
    assert not bad, bad
