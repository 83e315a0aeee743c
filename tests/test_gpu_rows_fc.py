"""GPU parity of the MinkowskiNet head's fc_layer (csn_amd/csrc/rows_fc.hip; include/csn_hip.h section 13) against the float64
restatement tests/rows_fc_ref.py, in math modes 0 and 1: the raw ABI at the row-tile edges and the three backbone widths, at natural
and at padded pitches, determinism, a dead column, the ``BackboneFC`` module through autograd, and ``SimCSNHead`` with
``backbone_channels`` against "float64 fc, then the float64 head".

Bounds (the project's contract): y, mean and the running statistics within 1e-4 absolute; gradients within 1e-4 of each tensor's
max, except where the true gradient nearly cancels (batches below 31 rows, and dbias in training mode, which is mathematically
zero): there the scale is the same contraction taken with absolute values of every term (rows_fc_ref.bwd).  The backward reference
is evaluated with the GPU's own ReLU mask (y_gpu > 0); the mask itself must equal the reference's wherever the float64
pre-activation is at least 1e-4 from zero, and at most 0.1 % of a case's elements may be nearer than that.

Measured on MI355X, maxima over the raw-ABI cases (fp32 / bf16x3): y 5.4e-6 / 3.4e-5 (the 2- and 3-row batches), z 4.4e-6 / 2.2e-5,
mean 7.6e-7 / 8.5e-6, running mean 1.7e-8 / 1.7e-7, running variance 1.0e-7 / 4.3e-7; N >= 31: dx 8.1e-7 / 8.4e-6, dw 2.6e-7 / 7.5e-6,
dgamma 5.6e-7 / 6.2e-6, dbeta 4.5e-8, dbias 1.0e-7; N < 31: dx 3.2e-7 / 2.9e-6, dw 7.7e-7 / 1.0e-5, dbias 1.5e-7 / 9.5e-8,
dgamma 1.6e-6 / 1.3e-5.  Module: every gradient <= 5.0e-7 / 5.7e-6.  Head: outputs 6.8e-7 / 7.9e-6, gradients <= 6.6e-7 / 3.3e-5."""
import functools

import numpy as np
import pytest
import torch

from tests import rows_fc_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.02
CASES = [(2, 32, 32), (3, 480, 256), (5, 416, 96), (31, 480, 256), (64, 480, 256), (65, 992, 256), (129, 480, 128), (257, 416, 64),
         (1031, 480, 256)]
CANARY = -777.25


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
def _case(n, c_in, c_out):
    """Inputs and the float64 forward of one case, computed once and shared (never modified)."""
    i = R.inputs(1000 + n + c_in + c_out, n, c_in, c_out)
    f = {t: R.fwd(i["x"], i["w"], i["b"], i["gamma"], i["beta"], i["running_mean"], i["running_var"], EPS, MOM, t)
         for t in (True, False)}
    return i, f


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

    def __init__(self, L, i, n, c_in, c_out, training, pad=0):
        lib = L.lib()
        self.n, self.c_in, self.c_out, self.training, self.pad, self.L = n, c_in, c_out, training, pad, L
        d = lambda k: i[k].cuda().contiguous()
        self.x, self.xbuf = _rows(i["x"], pad, 1e30)
        self.w, self.b, self.gamma, self.beta = d("w"), d("b"), d("gamma"), d("beta")
        self.rm, self.rv = d("running_mean").clone(), d("running_var").clone()
        blank = torch.zeros(n, c_out)
        self.y, self.ybuf = _rows(blank, pad, CANARY)
        self.z, self.zbuf = _rows(blank, pad, CANARY)
        self.mean = torch.empty(c_out, device="cuda")
        self.invstd = torch.empty(c_out, device="cuda")
        wb = lib.csn_rows_fc_workspace_bytes(n, c_in, c_out, int(training), 0)
        ws = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.csn_rows_fc_fwd_f32(_ptr(self.x), c_in + pad, n, c_in, c_out, _ptr(self.w), _ptr(self.b), _ptr(self.gamma),
                                        _ptr(self.beta), _ptr(self.rm), _ptr(self.rv), EPS, MOM, int(training), _ptr(self.y),
                                        c_out + pad, _ptr(self.z) if training else None, c_out + pad,
                                        _ptr(self.mean) if training else None, _ptr(self.invstd) if training else None,
                                        _ptr(ws) if training else None, wb, st), "fwd")

    def backward(self, dy_cpu, want=("dx", "dw", "dbias")):
        lib, n, c_in, c_out, pad = self.L.lib(), self.n, self.c_in, self.c_out, self.pad
        self.dy, _ = _rows(dy_cpu, pad, 1e30)
        self.dx, self.dxbuf = _rows(torch.zeros(n, c_in), pad, CANARY)
        self.dw = torch.full((c_out, c_in), CANARY, device="cuda")
        self.dbias = torch.full((c_out,), CANARY, device="cuda")
        self.dgamma = torch.empty(c_out, device="cuda")
        self.dbeta = torch.empty(c_out, device="cuda")
        if not pad:
            self.dx.fill_(CANARY)
        wb = lib.csn_rows_fc_workspace_bytes(n, c_in, c_out, int(self.training), 1)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        sm, ss = (self.mean, self.invstd) if self.training else (self.rm, self.rv)
        st = torch.cuda.current_stream().cuda_stream
        self.L.check(lib.csn_rows_fc_bwd_f32(_ptr(self.dy), c_out + pad, _ptr(self.y), c_out + pad,
                                             _ptr(self.z) if self.training else None, c_out + pad, _ptr(self.x), c_in + pad, n, c_in,
                                             c_out, _ptr(self.w), _ptr(self.b), _ptr(self.gamma), _ptr(sm), _ptr(ss), EPS,
                                             int(self.training), _ptr(self.dx) if "dx" in want else None, c_in + pad,
                                             _ptr(self.dw) if "dw" in want else None, _ptr(self.dbias) if "dbias" in want else None,
                                             _ptr(self.dgamma), _ptr(self.dbeta), _ptr(ws), wb, st), "bwd")
        return self


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


def _check_backward(tag, run, i, f, n):
    """The gradients of ``run`` against the float64 reference under the GPU's own mask; returns the relative figures."""
    mask = run.y.cpu() > 0
    b = R.bwd(i["dy"], mask, i["x"], i["w"], i["gamma"], f, run.training)
    small = n < 31
    scale = {"dx": b["scale_dx"] if small else b["dx"].abs().max(), "dw": b["scale_dw"] if small else b["dw"].abs().max(),
             "dbias": b["scale_dbias"] if (small or run.training) else b["dbias"].abs().max(),
             "dgamma": b["dgamma"].abs().max(), "dbeta": b["dbeta"].abs().max()}
    got = {"dx": run.dx, "dw": run.dw, "dbias": run.dbias, "dgamma": run.dgamma, "dbeta": run.dbeta}
    e = {k: _err(got[k], b[k]) / max(float(scale[k]), 1e-30) for k in got}
    print(f"[rows_fc] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
    assert max(e.values()) < 1e-4, e
    return e


@pytest.mark.parametrize("pad", [0, 4], ids=["natural", "padded"])
@pytest.mark.parametrize("n,c_in,c_out", CASES, ids=[f"{a}x{b}x{c}" for a, b, c in CASES])
def test_raw_abi_against_float64(L, math_mode, n, c_in, c_out, pad):
    """Forward (training and eval), the ReLU mask and the backward of one case (measured maxima: module docstring)."""
    i, fs = _case(n, c_in, c_out)
    for training in (True, False):
        f = fs[training]
        run = Run(L, i, n, c_in, c_out, training, pad)
        tag = f"mode {math_mode} {n}x{c_in}x{c_out} pad {pad} {'train' if training else 'eval'}"
        e = {"y": _err(run.y, f["y"])}
        if training:
            e.update(mean=_err(run.mean, f["mean"]), rm=_err(run.rm, f["running_mean"]), rv=_err(run.rv, f["running_var"]),
                     z=_err(run.z, f["z"]))
        else:
            assert torch.equal(run.rm.cpu(), i["running_mean"]) and torch.equal(run.rv.cpu(), i["running_var"])
        decided = f["a"].abs() >= 1e-4
        undecided = 1.0 - decided.double().mean().item()
        print(f"[rows_fc] {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" undecided {undecided:.2e}")
        assert max(e.values()) < 1e-4, e
        assert undecided <= 1e-3
        assert torch.equal((run.y.cpu() > 0)[decided], (f["a"] > 0)[decided])
        run.backward(i["dy"])
        _check_backward(tag, run, i, f, n)
        if pad:
            assert _pad_intact(run.ybuf, n, c_out, pad, CANARY) and _pad_intact(run.dxbuf, n, c_in, pad, CANARY)
            assert _pad_intact(run.xbuf, n, c_in, pad, 1e30)
            if training:
                assert _pad_intact(run.zbuf, n, c_out, pad, CANARY)
            else:
                assert _pad_intact(run.zbuf, n, c_out, pad, CANARY) and bool((run.z == 0).all())     # eval writes nothing but y


def test_null_gradient_pointers_are_skipped(L, math_mode):
    n, c_in, c_out = 129, 480, 128
    i, fs = _case(n, c_in, c_out)
    full = Run(L, i, n, c_in, c_out, True).backward(i["dy"])
    for skip in ("dx", "dw", "dbias"):
        want = tuple(k for k in ("dx", "dw", "dbias") if k != skip)
        part = Run(L, i, n, c_in, c_out, True).backward(i["dy"], want=want)
        assert bool((getattr(part, skip) == CANARY).all()), skip
        for k in want + ("dgamma", "dbeta"):
            assert torch.equal(getattr(part, k), getattr(full, k)), (skip, k)
    none = Run(L, i, n, c_in, c_out, True).backward(i["dy"], want=())
    assert torch.equal(none.dgamma, full.dgamma) and torch.equal(none.dbeta, full.dbeta)
    assert bool((none.dx == CANARY).all()) and bool((none.dw == CANARY).all()) and bool((none.dbias == CANARY).all())


def test_two_calls_give_the_same_bits(L, math_mode):
    n, c_in, c_out = 1031, 480, 256
    i, _ = _case(n, c_in, c_out)
    a = Run(L, i, n, c_in, c_out, True).backward(i["dy"])
    b = Run(L, i, n, c_in, c_out, True).backward(i["dy"])
    for k in ("y", "z", "mean", "invstd", "rm", "rv", "dx", "dw", "dbias", "dgamma", "dbeta"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_dead_column(L, math_mode):
    """A column whose pre-activations are all negative: y = 0, no gradient to its gamma, beta, bias or weight row, all finite."""
    n, c_in, c_out = 65, 416, 96
    i = dict(_case(n, c_in, c_out)[0])
    i["beta"] = i["beta"].clone()
    i["beta"][3] = -50.0
    run = Run(L, i, n, c_in, c_out, True).backward(i["dy"])
    assert bool((run.y[:, 3] == 0).all())
    assert run.dgamma[3] == 0 and run.dbeta[3] == 0 and run.dbias[3] == 0 and bool((run.dw[3] == 0).all())
    for k in ("y", "z", "mean", "invstd", "rm", "rv", "dx", "dw", "dbias", "dgamma", "dbeta"):
        assert torch.isfinite(getattr(run, k)).all(), k
    f = R.fwd(i["x"], i["w"], i["b"], i["gamma"], i["beta"], i["running_mean"], i["running_var"], EPS, MOM, True)
    assert _err(run.y, f["y"]) < 1e-4
    _check_backward(f"mode {math_mode} dead column", run, i, f, n)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_module_through_autograd(L, math_mode, training):
    from csn_amd.minkowski_csn import BackboneFC
    n, c_in, c_out = 129, 480, 128
    i, fs = _case(n, c_in, c_out)
    f = fs[training]
    m = BackboneFC(c_in, c_out, bn_momentum=MOM, eps=EPS)
    with torch.no_grad():
        m[0].weight.copy_(i["w"]); m[0].bias.copy_(i["b"]); m[1].weight.copy_(i["gamma"]); m[1].bias.copy_(i["beta"])
        m[1].running_mean.copy_(i["running_mean"]); m[1].running_var.copy_(i["running_var"])
    m = m.cuda().train(training)
    x = i["x"].cuda().requires_grad_(True)
    y = m(x)
    (y * i["dy"].cuda()).sum().backward()
    assert int(m[1].num_batches_tracked) == (1 if training else 0)
    assert _err(y, f["y"]) < 1e-4
    assert _err(m[1].running_mean, f["running_mean"]) < 1e-4 and _err(m[1].running_var, f["running_var"]) < 1e-4
    b = R.bwd(i["dy"], y.detach().cpu() > 0, i["x"], i["w"], i["gamma"], f, training)
    got = {"dx": x.grad, "dw": m[0].weight.grad, "dbias": m[0].bias.grad, "dgamma": m[1].weight.grad, "dbeta": m[1].bias.grad}
    scale = {k: b[k].abs().max() for k in got}
    if training:
        scale["dbias"] = b["scale_dbias"]
    e = {k: _err(got[k], b[k]) / float(scale[k]) for k in got}
    print(f"[rows_fc] module mode {math_mode} {'train' if training else 'eval'}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) < 1e-4, e
    if training:
        with pytest.raises(ValueError):
            m(x[:1])
    # no gradient asked of the rows: dx is skipped, the parameter gradients are the same bits
    m.zero_grad()
    m[1].running_mean.copy_(i["running_mean"]); m[1].running_var.copy_(i["running_var"])
    (m(i["x"].cuda()) * i["dy"].cuda()).sum().backward()
    assert torch.equal(m[0].weight.grad, got["dw"])


# ------------------------------------------------------------------------------------------------------
# the head with backbone_channels
# ------------------------------------------------------------------------------------------------------
HEAD_SEED = 2                           # chosen on the CPU: the float64 fc pre-activations of this seed are all >= 1.7e-4 from zero
H_C, H_IN, H_HEADS, H_K, H_OUT = 32, 416, 2, 2, 11
H_QLENS, H_KLENS = (37, 64, 5), ((5, 37, 64), (64, 1, 37))


def head_case(seed):
    """Parameters (SimCSNHead names, float32 CPU) and ragged backbone rows of the head test."""
    from tests.test_gpu_minkowski_csn import _params
    rng = np.random.default_rng(seed)
    p = _params(rng, H_HEADS, H_C, H_OUT, H_K)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    p["fc_layer.0.weight"] = t(rng.standard_normal((H_C, H_IN)) / np.sqrt(H_IN))
    p["fc_layer.0.bias"] = t(0.1 * rng.standard_normal(H_C))
    p["fc_layer.1.weight"] = t(1 + 0.2 * rng.standard_normal(H_C))
    p["fc_layer.1.bias"] = t(0.3 * rng.standard_normal(H_C))
    p["fc_layer.1.running_mean"] = t(0.1 * rng.standard_normal(H_C))
    p["fc_layer.1.running_var"] = t(1 + 0.1 * np.abs(rng.standard_normal(H_C)))
    p["fc_layer.1.num_batches_tracked"] = torch.tensor(0)
    shape = lambda n: t(rng.standard_normal((n, H_IN)) + 0.8 * rng.standard_normal((1, H_IN)))
    qs = [shape(n) for n in H_QLENS]
    keys = [[shape(m) for m in ms] for ms in H_KLENS]
    g = t(rng.standard_normal((sum(H_QLENS), H_OUT)))
    return p, qs, keys, g


def ref_fc_batches(p64, batches):
    """float64 fc_layer in training mode on the batches in order (each a list of per-shape rows): the per-shape outputs, the
    forward dicts of rows_fc_ref.fwd (their y keeps its gradient) and the running statistics after the last batch."""
    rm, rv = p64["fc_layer.1.running_mean"], p64["fc_layer.1.running_var"]
    outs, fwds = [], []
    for shapes in batches:
        f = R.fwd(torch.cat(shapes), p64["fc_layer.0.weight"], p64["fc_layer.0.bias"], p64["fc_layer.1.weight"],
                  p64["fc_layer.1.bias"], rm, rv, EPS, MOM, True)
        rm, rv = f["running_mean"], f["running_var"]
        if f["y"].requires_grad:
            f["y"].retain_grad()
        outs.append(list(torch.split(f["y"], [s.shape[0] for s in shapes])))
        fwds.append(f)
    return outs, fwds, rm, rv


def test_head_with_backbone_rows_against_float64(L, math_mode):
    """Train mode (BatchNorm over each batch, dropout 0): outputs within 1e-4 absolute; gradients to the backbone rows of the
    queries and of every key batch and to every parameter within 1e-4 of each tensor's max; the running statistics are three
    momentum updates in query, key 0, key 1 order."""
    from csn_amd.minkowski_csn import SimCSNHead
    from tests.test_gpu_minkowski_csn import _pack, _rel, ref_head
    p, qs, keys, g = head_case(HEAD_SEED)
    float_names = [n for n, t in p.items() if t.dtype.is_floating_point and "running" not in n]
    p64 = {n: (t.double().requires_grad_(True) if n in float_names else t.double()) for n, t in p.items()}
    q64 = [t.double().requires_grad_(True) for t in qs]
    k64 = [[t.double().requires_grad_(True) for t in ks] for ks in keys]
    outs, fwds, rm, rv = ref_fc_batches(p64, [q64] + k64)
    assert min(f["a"].detach().abs().min().item() for f in fwds) >= 1e-4     # the reference's own mask is decided everywhere
    ref = ref_head(outs[0], outs[1:], p64, H_HEADS, H_C)
    (ref * g.double()).sum().backward()
    # the convolution's bias gradient is mathematically zero under a training-mode BatchNorm: its scale is the sum of the
    # absolute values of the terms that cancel, over the three batches (rows_fc_ref.bwd), never max|ref|
    with torch.no_grad():
        bias_scale = sum(R.bwd(f["y"].grad, f["a"] > 0, torch.cat(b), p64["fc_layer.0.weight"], p64["fc_layer.1.weight"],
                               {k: v.detach() for k, v in f.items()}, True)["abs_dbias"]
                         for f, b in zip(fwds, [q64] + k64)).max().item()

    head = SimCSNHead(H_C, H_HEADS, H_OUT, H_K, dropout=0.0, backbone_channels=H_IN, bn_momentum=MOM)
    head.load_state_dict(p)
    head = head.cuda().train()
    head.MHA.dropout.p = 0.0
    head.MHA.attention.dropout.p = 0.0                                    # (the attention's own rate is not a constructor argument)
    q, qo = _pack(qs)
    qd = q.cuda().requires_grad_(True)
    kd = [(_pack(ks)[0].cuda().requires_grad_(True), _pack(ks)[1]) for ks in keys]
    out = head(qd, qo, kd)
    assert out.shape == (sum(H_QLENS), H_OUT)
    (out * g.cuda()).sum().backward()
    bn = head.fc_layer[1]
    assert int(bn.num_batches_tracked) == 3
    assert _err(bn.running_mean, rm.detach()) < 1e-4 and _err(bn.running_var, rv.detach()) < 1e-4

    e_out = _err(out, ref.detach())
    e = {"dq": _rel(qd.grad, torch.cat([t.grad for t in q64]))}
    for j, ks in enumerate(k64):
        e[f"dk{j}"] = _rel(kd[j][0].grad, torch.cat([t.grad for t in ks]))
    for name, prm in head.named_parameters():
        e[name] = _rel(prm.grad, p64[name].grad)
    e["fc_layer.0.bias"] = _err(head.fc_layer[0].bias.grad, p64["fc_layer.0.bias"].grad) / bias_scale
    print(f"[rows_fc] head mode {math_mode}: out {e_out:.1e} " + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
    assert e_out < 1e-4
    assert max(e.values()) < 1e-4, e

    # return_ssa: only the queries pass through fc_layer (one more batch), shape_ssa works through head(...)
    from csn_amd.minkowski_csn import shape_ssa
    rows, off = shape_ssa(head, [t.cuda() for t in qs])
    assert rows.shape == (sum(H_QLENS), H_C) and off == qo and int(bn.num_batches_tracked) == 4


def test_head_without_backbone_channels_is_unchanged(L, math_mode):
    from csn_amd.minkowski_csn import SimCSNHead
    torch.manual_seed(11)
    a = SimCSNHead(32, 2, 5, 1).cuda().eval()
    b = SimCSNHead(32, 2, 5, 1, backbone_channels=None, bn_momentum=0.5)
    assert sorted(a.state_dict()) == sorted(b.state_dict())
    b.load_state_dict(a.state_dict())
    b = b.cuda().eval()
    g = torch.Generator().manual_seed(12)
    q = torch.randn(42, 32, generator=g).cuda()
    k = torch.randn(30, 32, generator=g).cuda()
    with torch.no_grad():
        assert torch.equal(a(q, [0, 37, 42], [(k, [0, 5, 30])]), b(q, [0, 37, 42], [(k, [0, 5, 30])]))
