"""GPU parity of the gather-GEMM with a BatchNorm statistics epilogue over a concatenation that is never formed
(csn_amd/csrc/sparse_conv_cat.hip; include/csn_hip.h section 27; ``csn_amd.cat_conv_stats``) in math modes 0 and 1 against float64 on
the concatenation (tests/sparse_conv_ref.py ``fwd`` / ``bwd``, tests/hrnet_ref.py ``stats``): parts (256, 128), (256, 32), (32, 256),
(128, 32, 64) and a single (96), kernel 3 and kernel 1, on ``random_set(129)``, ``random_set(1031)`` and ``two_clusters`` (a last tile
that skips every offset but the centre), at natural and padded pitches and with the parts handed over as column blocks of one wider
buffer; every instance of the accumulating kernel (column blocks per wave pinned by ``CSN_DEV_SCONV_NB``); one part bit for bit
against ``conv_stats``; determinism; ``dx`` per part and ``dw`` through autograd; the host refusals; the single-product instances
(``rows_single_product``, modes bf16 / fp16) against the rounding bound of their operands.

Bounds: z within 1e-4 of float64 (weights of variance 1 / (KV sum c_in), outputs O(1): the project's contract for the gather-GEMM);
the statistics as tests/test_gpu_hrnet.py holds (15a): mean 1e-4, invstd 1e-4 max(invstd, invstd^2), running statistics 1e-4; each
gradient within 1e-4 of its tensor's max.  Single product: every operand is rounded once to 8 (bf16) or 11 (fp16) significant bits,
so a product errs by at most 2 u + u^2 of its magnitude, u = 2^-8 / 2^-11: |z - z64| <= 2.1 u sum |x| |w| + 1e-4.

Measured on MI355X, maxima over the cases (fp32 / bf16x3; every test prints its own).  Raw ABI, all sets, parts and kernel sizes: z
8.1e-6 / 2.4e-5, mean 8.0e-8 / 1.3e-6, invstd 1.9e-7 / 1.5e-6, running mean 3.0e-8 / 1.3e-7, running variance 7.7e-8 / 3.2e-7.  Pitched
parts and a padded result: z 6.7e-7 / 6.1e-6.  Column blocks pinned to 1 .. 4: z 3.2e-6 / 9.7e-6.  Through autograd: z 1.9e-6 / 1.8e-5, dw
1.2e-7 / 5.6e-6, dx per part <= 5.5e-7 / 6.1e-6.  Single product: z 2.4e-3 (bf16, bound >= 1.3e-2) and 3.1e-4 (fp16, bound >= 1.8e-3)."""
import ctypes
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
MOM = 0.1
SETS = {"rand129": lambda: R.random_set(129), "rand1031": lambda: R.random_set(1031), "clusters": R.two_clusters}
PARTS = [(256, 128), (256, 32), (32, 256), (128, 32, 64), (96,)]
E_ARG, E_ALIGN, E_PTR, E_DIM, E_WORKSPACE = -1, -2, -3, -5, -6


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
def _geometry(name, k):
    from csn_amd.minkowski_conv import build_kernel_map
    pts = SETS[name]()
    return R.geometry("s1", pts, k=k)[0], build_kernel_map(torch.tensor(pts), kernel_size=k, stride=1, tensor_stride=1)


@functools.lru_cache(maxsize=None)
def _case(name, k, parts, c_out):
    """Inputs and the float64 forward, statistics and backward on the concatenation: computed once, shared, never modified."""
    g, m = _geometry(name, k)
    t = R.tensors(len(name) + k + sum(parts) + 3 * c_out + len(parts), g.n_in, g.n_out, g.KV, sum(parts), c_out)
    gen = torch.Generator().manual_seed(c_out + g.n_out)
    rm, rv = 0.3 * torch.randn(c_out, generator=gen), 0.5 + torch.rand(c_out, generator=gen)
    z = R.fwd(g, t["x"], t["w"])
    return g, m, t, rm, rv, z, H.stats(z, momentum=MOM, running_mean=rm, running_var=rv), R.bwd(g, t["dy"], t["x"], t["w"])


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _split(x, parts, layout):
    """The parts of x (n, sum parts) on the device: "natural" contiguous tensors, "padded" views of pitch c + 12 starting 16 bytes
    into their buffers (the padding holds 1e30), "blocks" column blocks of ONE (n, sum parts) buffer."""
    xs, c0 = [], 0
    whole = x.cuda().contiguous()
    for c in parts:
        piece = x[:, c0:c0 + c]
        if layout == "natural":
            xs.append(piece.cuda().contiguous())
        elif layout == "blocks":
            xs.append(whole[:, c0:c0 + c])
        else:
            buf = torch.full((4 + x.shape[0] * (c + 12),), 1e30, dtype=torch.float32, device="cuda")
            view = buf[4:].view(x.shape[0], c + 12)
            view[:, :c] = piece.cuda()
            xs.append(view[:, :c])
        c0 += c
    return xs


class Run:
    """One call of section 27 through the raw ABI."""

    def __init__(self, L, m, t, parts, rm, rv, layout="natural", zpad=0, ws_short=0, expect=0, n_parts=None, kv=None, widths=None,
                 x_off=0):
        lib = L.lib()
        mm = m.to("cuda")
        KV, _, c_out = t["w"].shape
        self.xs = _split(t["x"], parts, layout)
        self.w = t["w"].cuda().contiguous()
        n_out = m.n_out
        self.zbuf = torch.full((4 + n_out * (c_out + zpad),), CANARY, dtype=torch.float32, device="cuda")
        self.z = self.zbuf[4:].view(n_out, c_out + zpad)[:, :c_out]
        self.mean, self.invstd = torch.full((c_out,), CANARY, device="cuda"), torch.full((c_out,), CANARY, device="cuda")
        self.rm, self.rv = rm.cuda().clone(), rv.cuda().clone()
        cp = L.CatParts()
        for i, x in enumerate(self.xs):
            cp.x[i], cp.ld_x[i], cp.c_in[i] = x.data_ptr() + x_off, x.stride(0), (widths or parts)[i]
        wb = lib.csn_sparse_conv_cat_stats_workspace_bytes(n_out, c_out)
        assert wb > 0
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        self.status = lib.csn_sparse_conv_cat_stats_fwd_f32(ctypes.byref(cp), len(parts) if n_parts is None else n_parts, m.n_in,
                                                            _ptr(mm.fwd), n_out, KV if kv is None else kv, c_out, _ptr(self.w),
                                                            _ptr(self.z), c_out + zpad, _ptr(self.mean), _ptr(self.invstd),
                                                            _ptr(self.rm), _ptr(self.rv), H.EPS, MOM, _ptr(ws), wb - ws_short, _st())
        assert self.status == expect, self.status
        self.n_out, self.c_out, self.zpad = n_out, c_out, zpad

    def untouched(self, rm, rv):
        return (bool((self.zbuf == CANARY).all()) and bool((self.mean == CANARY).all()) and bool((self.invstd == CANARY).all())
                and torch.equal(self.rm.cpu(), rm) and torch.equal(self.rv.cpu(), rv))

    def pad_intact(self):
        full = self.zbuf[4:].view(self.n_out, self.c_out + self.zpad)
        return bool((self.zbuf[:4] == CANARY).all()) and bool((full[:, self.c_out:] == CANARY).all())


def _check(tag, run, z, ref):
    e = {"z": (run.z.cpu().double() - z).abs().max().item(),
         "mean": (run.mean.cpu().double() - ref["mean"]).abs().max().item(),
         "invstd": ((run.invstd.cpu().double() - ref["invstd"]).abs() / torch.maximum(ref["invstd"], ref["invstd"] ** 2)).max().item(),
         "rmean": (run.rm.cpu().double() - ref["running_mean"]).abs().max().item(),
         "rvar": (run.rv.cpu().double() - ref["running_var"]).abs().max().item()}
    print(f"[cat stats] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert torch.isfinite(run.z).all()
    assert max(e.values()) < 1e-4, e
    return e


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("parts", PARTS, ids=["+".join(map(str, p)) for p in PARTS])
@pytest.mark.parametrize("name", list(SETS))
def test_raw_abi_against_float64_on_the_concatenation(L, math_mode, name, parts, k):
    c_out = 256 if parts == (256, 128) else 64
    g, m, t, rm, rv, z, ref, _ = _case(name, k, parts, c_out)
    _check(f"mode {math_mode} {name} k {k} parts {parts} -> {c_out}", Run(L, m, t, parts, rm, rv), z, ref)


@pytest.mark.parametrize("layout", ["padded", "blocks"])
@pytest.mark.parametrize("parts", [(256, 32), (128, 32, 64)], ids=["256+32", "128+32+64"])
def test_pitched_parts_and_a_padded_result(L, math_mode, parts, layout):
    g, m, t, rm, rv, z, ref, _ = _case("rand129", 3, parts, 64)
    run = Run(L, m, t, parts, rm, rv, layout=layout, zpad=12)
    _check(f"mode {math_mode} rand129 parts {parts} {layout}", run, z, ref)
    assert run.pad_intact()
    assert torch.equal(run.z, Run(L, m, t, parts, rm, rv).z)                   # the pitch changes no bit


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_every_instance_of_the_accumulating_kernel(L, math_mode, nb):
    g, m, t, rm, rv, z, ref, _ = _case("rand1031", 3, (32, 256), 128)
    L.lib().csn_dev_set(L.DEV_SCONV_NB, nb)
    try:
        _check(f"mode {math_mode} rand1031 parts (32, 256) -> 128 NB {nb}", Run(L, m, t, (32, 256), rm, rv), z, ref)
    finally:
        L.lib().csn_dev_set(L.DEV_SCONV_NB, 0)


@pytest.mark.parametrize("k", [3, 1])
def test_one_part_is_conv_stats_and_two_calls_give_the_same_bits(L, math_mode, k):
    import csn_amd
    from csn_amd import functional as CF
    g, m, t, rm, rv, _, _, _ = _case("rand1031", k, (96,), 64)
    one = Run(L, m, t, (96,), rm, rv)
    rm_d, rv_d = rm.cuda().clone(), rv.cuda().clone()
    with CF.math_mode(math_mode):
        z, mean, invstd = csn_amd.conv_stats(t["x"].cuda(), t["w"].cuda(), m.to("cuda"), rm_d, rv_d, H.EPS, MOM)
    for a, b in ((one.z, z), (one.mean, mean), (one.invstd, invstd), (one.rm, rm_d), (one.rv, rv_d)):
        assert torch.equal(a, b)
    g, m, t, rm, rv, _, _, _ = _case("rand1031", k, (128, 32, 64), 64)
    a, b = Run(L, m, t, (128, 32, 64), rm, rv), Run(L, m, t, (128, 32, 64), rm, rv)
    for q in ("z", "mean", "invstd", "rm", "rv"):
        assert torch.equal(getattr(a, q), getattr(b, q)), q


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("parts", [(256, 128), (128, 32, 64)], ids=["256+128", "128+32+64"])
def test_autograd_gradients_per_part(L, math_mode, parts, k):
    import csn_amd
    from csn_amd import functional as CF
    c_out = 64
    g, m, t, rm, rv, z64, ref, b = _case("rand129", k, parts, c_out)
    whole = t["x"].cuda()
    xs, c0 = [], 0
    for c in parts:                                                          # leaves that are column blocks of one buffer
        xs.append(whole[:, c0:c0 + c].detach().requires_grad_(True))
        c0 += c
    w = t["w"].cuda().requires_grad_(True)
    rm_d, rv_d = rm.cuda().clone(), rv.cuda().clone()
    with CF.math_mode(math_mode):
        z, mean, invstd = csn_amd.cat_conv_stats(xs, w, m.to("cuda"), rm_d, rv_d, H.EPS, MOM)
        assert not mean.requires_grad and not invstd.requires_grad
        z.backward(t["dy"].cuda())
    e = {"z": (z.detach().cpu().double() - z64).abs().max().item(),
         "dw": (w.grad.cpu().double() - b["dw"]).abs().max().item() / b["dw"].abs().max().item()}
    c0 = 0
    for i, c in enumerate(parts):
        want = b["dx"][:, c0:c0 + c]
        e[f"dx{i}"] = (xs[i].grad.cpu().double() - want).abs().max().item() / want.abs().max().item()
        c0 += c
    print(f"[cat stats] autograd mode {math_mode} k {k} parts {parts}: " + " ".join(f"{q} {v:.1e}" for q, v in e.items()))
    assert max(e.values()) < 1e-4, e
    assert (rm_d.cpu().double() - ref["running_mean"]).abs().max() < 1e-4 and (rv_d.cpu().double() - ref["running_var"]).abs().max() < 1e-4
    # needs_input_grad: only the first part asks for a gradient
    x0 = xs[0].detach().requires_grad_(True)
    with CF.math_mode(math_mode):
        z2, _, _ = csn_amd.cat_conv_stats([x0] + [x.detach() for x in xs[1:]], w.detach(), m.to("cuda"), None, None, H.EPS, MOM)
        z2.backward(t["dy"].cuda())
    assert torch.equal(z2.detach(), z.detach()) and torch.equal(x0.grad, xs[0].grad)


def test_host_refusals_leave_every_output_untouched(L, math_mode):
    g, m, t, rm, rv, _, _, _ = _case("rand129", 3, (256, 32), 64)
    parts = (256, 32)
    assert Run(L, m, t, parts, rm, rv, ws_short=16, expect=E_WORKSPACE).untouched(rm, rv)
    assert Run(L, m, t, parts, rm, rv, n_parts=0, expect=E_ARG).untouched(rm, rv)
    assert Run(L, m, t, parts, rm, rv, n_parts=5, expect=E_ARG).untouched(rm, rv)
    assert Run(L, m, t, parts, rm, rv, kv=125, expect=E_DIM).untouched(rm, rv)
    assert Run(L, m, t, parts, rm, rv, widths=(240, 48), expect=E_DIM).untouched(rm, rv)     # widths that are no multiples of 32
    assert Run(L, m, t, parts, rm, rv, widths=(288, 32), expect=E_DIM).untouched(rm, rv)     # a part wider than 256
    assert Run(L, m, t, parts, rm, rv, x_off=4, expect=E_PTR).untouched(rm, rv)              # a part that is not 16-byte aligned
    assert Run(L, m, t, parts, rm, rv, zpad=2, expect=E_ALIGN).untouched(rm, rv)             # a pitch that is no multiple of 4
    # a one-row batch
    from csn_amd.minkowski_conv import build_kernel_map
    one = build_kernel_map(torch.tensor(R.single_voxel()), kernel_size=3, stride=1, tensor_stride=1)
    t1 = R.tensors(3, 1, 1, 27, 288, 64)
    assert Run(L, one, t1, parts, rm, rv, expect=E_ARG).untouched(rm, rv)


def test_python_refusals(L):
    import csn_amd
    from csn_amd._lib import CsnError
    from csn_amd.minkowski_conv import build_kernel_map
    m = build_kernel_map(torch.tensor(R.random_set(129)), kernel_size=3, stride=1, tensor_stride=1)
    with pytest.raises(CsnError):
        csn_amd.cat_conv_stats([torch.zeros(129, 32), torch.zeros(129, 32)], torch.zeros(27, 64, 32), m, None, None, 1e-5, 0.1)
    one = build_kernel_map(torch.tensor(R.single_voxel()), kernel_size=3, stride=1, tensor_stride=1).to("cuda")
    with pytest.raises(ValueError, match="more than 1 value"):
        csn_amd.cat_conv_stats([torch.zeros(1, 32, device="cuda")] * 2, torch.zeros(27, 64, 32, device="cuda"), one, None, None, 1e-5, 0.1)
    md = m.to("cuda")
    with pytest.raises(ValueError):
        csn_amd.cat_conv_stats([torch.zeros(129, 32, device="cuda")] * 5, torch.zeros(27, 160, 32, device="cuda"), md, None, None, 1e-5, 0.1)
    with pytest.raises(ValueError):
        csn_amd.cat_conv_stats([torch.zeros(129, 48, device="cuda")] * 2, torch.zeros(27, 96, 32, device="cuda"), md, None, None, 1e-5, 0.1)


@pytest.mark.parametrize("mode,u", [("bf16", 2.0 ** -8), ("fp16", 2.0 ** -11)])
def test_single_product_instances_stay_inside_their_rounding_bound(L, mode, u):
    """``rows_single_product`` in modes bf16 / fp16 reaches the accumulating kernel's 16-bit instances (forward only)."""
    import csn_amd
    from csn_amd import functional as CF
    from csn_amd import tuning
    parts = (256, 32)
    g, m, t, rm, rv, z64, _, _ = _case("rand129", 3, parts, 64)
    mag = R.fwd(g, t["x"].abs(), t["w"].abs())
    xs = _split(t["x"], parts, "blocks")
    with CF.math_mode(mode), tuning.override(rows_single_product=True), torch.no_grad():
        z, mean, invstd = csn_amd.cat_conv_stats(xs, t["w"].cuda(), m.to("cuda"), None, None, H.EPS, MOM)
    err = (z.cpu().double() - z64).abs()
    print(f"[cat stats] single product {mode}: z {err.max().item():.1e} (bound {(2.1 * u * mag + 1e-4).min().item():.1e} ..)")
    assert bool((err <= 2.1 * u * mag + 1e-4).all())
    s = H.stats(z.cpu())
    assert (mean.cpu().double() - s["mean"]).abs().max() < 1e-4                 # the statistics are those of the z that was stored
    assert ((invstd.cpu().double() - s["invstd"]).abs() / torch.maximum(s["invstd"], s["invstd"] ** 2)).max() < 1e-4
