"""GPU parity of the Res16UNet family on voxel rows (csn_amd/minkowski_unet.py) against the float64 restatement tests/unet_ref.py:
the training forward, every gradient and the running statistics after one step, and the eval forward, of ``Res16UNet14`` (every
decoder block reads more than 256 columns: the split path) and ``Res16UNet14A`` (every decoder block at most 256: the cat path) on
300 voxels; the eval forward of ``Res16UNet34C`` on 1031 voxels; ``fused=True`` and ``fused=False`` alike; two ``SegTrainer``
iterations through ``train_seg.main`` and a resumed third.  All five levels of both point sets keep 16 rows or more
(tests/test_cpu_octant.py), so no BatchNorm is ill-conditioned by construction.

Bound for whole networks (the rule of tests/test_gpu_hrnet.py, with a yardstick that needs no model): the float64 restatement's own
graph, evaluated in float32 with torch ops on the device, is measured against float64; a model may be off by at most the larger of
1e-4 and twice that — outputs absolute, gradients relative to each tensor's max, running statistics absolute.  Gradients are taken
against float64 under each path's own ReLU masks (the yardstick's from its own pre-activations, a model's from its trace).  The
yardstick is an fp32 graph, so the models run in math mode 0, the exact fp32 products; in math mode 1 (bf16x3, the library's
default: three bf16 products for one fp32 product, per-product error about 2^-16 relative against fp32's 2^-24) an fp32 graph says
nothing about the arithmetic under test, and the rule of tests/test_gpu_hrnet.py is taken as it stands there: ``fused=True`` may be
off by at most the larger of 1e-4 and twice what ``fused=False`` (the octant nodes and ``sparse_conv3d`` + ATen) is in the same mode.

Measured on MI355X (every test prints its own).  Math mode 0, fp32 graph | fused | unfused: ``Res16UNet14`` training y 6.6e-6 | 1.3e-5 |
1.1e-5, gradients 2.9e-6 | 6.5e-6 | 5.5e-6, running statistics 1.4e-7 on all three; ``Res16UNet14A`` training y 4.0e-6 | 1.1e-5 | 8.7e-6,
gradients 2.1e-6 | 4.4e-6 | 5.5e-6; eval y 1.9e-7 .. 2.8e-7 | 2.1e-7 .. 3.5e-7 | 2.0e-7 .. 3.1e-7 over the three networks.  Math mode 1,
fused | unfused: ``Res16UNet14`` training y 1.7e-4 | 1.7e-4, gradients 6.0e-5 | 7.8e-5, running statistics 7.8e-7 | 7.8e-7;
``Res16UNet14A`` training y 1.4e-4 | 1.5e-4, gradients 6.6e-5 | 7.3e-5; eval y <= 4.9e-6 | 4.6e-6."""
import functools

import numpy as np
import pytest
import torch

from tests import sparse_conv_ref as R
from tests import unet_ref as U

pytestmark = pytest.mark.gpu

N_OUT = 6


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


def _set_mode(L, mode):
    L.check(L.lib().csn_set_math_mode(mode))


@pytest.fixture(autouse=True)
def _restore_mode(L):
    yield
    L.lib().csn_set_math_mode(1)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    pts = R.random_set(n)
    g = torch.Generator().manual_seed(n)
    return pts, U.Pyramid(pts), torch.randn(n, 3, generator=g), torch.randn(n, N_OUT, generator=g)


def _p64(net, grad=False):
    return {k: (v.double().requires_grad_(grad and "running" not in k) if v.is_floating_point() else v) for k, v in U.params(net).items()}


@functools.lru_cache(maxsize=None)
def reference(net, n, training):
    """(logits, pre-activations, new running statistics) of the float64 restatement with true ReLUs; shared, never modified."""
    _, pyr, feats, _ = _inputs(n)
    with torch.no_grad():
        return U.network(pyr, feats.double(), _p64(net), net, training)


def _masked_gradients(net, n, masks):
    """The float64 gradients of the training forward under the given ReLU masks."""
    _, pyr, feats, dy = _inputs(n)
    p = _p64(net, grad=True)
    f64 = feats.double().requires_grad_(True)
    y, _, _ = U.network(pyr, f64, p, net, True, masks=masks)
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    return dict(zip(["feats"] + names, torch.autograd.grad(y, [f64] + [p[k] for k in names], dy.double())))


def _errors(net, n, training, y, grads, masks, running):
    """y absolute; gradients relative to each tensor's max, under ``masks``; running statistics absolute."""
    ref_y, _, new = reference(net, n, training)
    e = {"y": (y.detach().cpu().double() - ref_y).abs().max().item(), "grad": 0.0, "running": 0.0, "grad_at": "-"}
    if grads is not None:
        want = _masked_gradients(net, n, masks)
        assert sorted(grads) == sorted(want) and all(v is not None for v in grads.values())
        rel = {k: (grads[k].detach().cpu().double() - w).abs().max().item() / max(w.abs().max().item(), 1e-300) for k, w in want.items()}
        e["grad_at"] = max(rel, key=rel.get)
        e["grad"] = rel[e["grad_at"]]
    for name, (rm, rv) in new.items():
        e["running"] = max(e["running"], (running[name + ".running_mean"].detach().cpu().double() - rm).abs().max().item(),
                           (running[name + ".running_var"].detach().cpu().double() - rv).abs().max().item())
    return e


@functools.lru_cache(maxsize=None)
def yardstick(net, n, training):
    """The restatement's graph in float32 with torch ops on the device, measured against float64."""
    _, pyr, feats, dy = _inputs(n)
    p = {k: (v.cuda().requires_grad_(training and "running" not in k) if v.is_floating_point() else v.cuda()) for k, v in U.params(net).items()}
    x = feats.cuda().requires_grad_(training)
    with torch.enable_grad() if training else torch.no_grad():
        y, pre, new = U.network(pyr, x, p, net, training)
    grads = None
    if training:
        names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
        grads = dict(zip(["feats"] + names, torch.autograd.grad(y, [x] + [p[k] for k in names], dy.cuda())))
    running = {}
    for name, (rm, rv) in new.items():
        running[name + ".running_mean"], running[name + ".running_var"] = rm, rv
    return _errors(net, n, training, y, grads, {k: v.detach().cpu() > 0 for k, v in pre.items()}, running)


def _run_model(net, n, training, fused):
    import csn_amd
    pts, _, feats, dy = _inputs(n)
    model = getattr(csn_amd, net)(3, N_OUT, fused=fused).cuda().train(training)
    model.load_state_dict(U.params(net))
    pyr = csn_amd.build_unet_pyramid(torch.tensor(pts)).to("cuda")
    x = feats.cuda().requires_grad_(training)
    trace = {}
    with torch.enable_grad() if training else torch.no_grad():
        y = model((pyr, x), trace)
    assert y.shape == (n, N_OUT) and sorted(trace) == sorted(reference(net, n, training)[1])
    grads = None
    if training:
        y.backward(dy.cuda())
        grads = {"feats": x.grad, **{k: v.grad for k, v in model.named_parameters()}}
    sd = model.state_dict()
    for name in reference(net, n, training)[2]:
        assert int(sd[name + ".num_batches_tracked"]) == (1 if training else 0), name
    return _errors(net, n, training, y, grads, {k: v.cpu() > 0 for k, v in trace.items()}, sd)


def _show(tag, e):
    return f"{tag} y {e['y']:.1e} gradients {e['grad']:.1e} ({e['grad_at']}) running {e['running']:.1e}"


CASES = [("Res16UNet14", 300, True), ("Res16UNet14", 300, False), ("Res16UNet14A", 300, True), ("Res16UNet14A", 300, False),
         ("Res16UNet34C", 1031, False)]


@pytest.mark.parametrize("net,n,training", CASES, ids=[f"{a}-{n}-{'train' if t else 'eval'}" for a, n, t in CASES])
def test_network_against_float64(L, net, n, training):
    yard = yardstick(net, n, training)
    _set_mode(L, 0)
    fused, plain = _run_model(net, n, training, True), _run_model(net, n, training, False)
    print(f"[unet] {net} n {n} {'train' if training else 'eval'} fp32: " + " | ".join(
        _show(t, e) for t, e in (("fp32 graph", yard), ("fused", fused), ("unfused", plain))))
    for q in ("y", "grad", "running"):
        assert fused[q] <= max(1e-4, 2 * yard[q]), ("fused", q, fused[q], yard[q])
        assert plain[q] <= max(1e-4, 2 * yard[q]), ("unfused", q, plain[q], yard[q])


@pytest.mark.parametrize("net,n,training", CASES, ids=[f"{a}-{n}-{'train' if t else 'eval'}" for a, n, t in CASES])
def test_fused_against_unfused_in_bf16x3(L, net, n, training):
    _set_mode(L, 1)
    fused, plain = _run_model(net, n, training, True), _run_model(net, n, training, False)
    print(f"[unet] {net} n {n} {'train' if training else 'eval'} bf16x3: " + " | ".join(
        _show(t, e) for t, e in (("fused", fused), ("unfused", plain))))
    for q in ("y", "grad", "running"):
        assert fused[q] <= max(1e-4, 2 * plain[q]), (q, fused[q], plain[q])


def test_model_takes_coordinates_and_a_voxel_pyramid(L):
    import csn_amd
    pts, _, feats, _ = _inputs(300)
    model = csn_amd.Res16UNet14A(3, N_OUT).cuda().eval()
    model.load_state_dict(U.params("Res16UNet14A"))
    coords = torch.tensor(pts)
    with torch.no_grad():
        a = model((csn_amd.build_unet_pyramid(coords).to("cuda"), feats.cuda()))
        b = model((coords.cuda(), feats.cuda()))
        c = model((csn_amd.build_pyramid(coords, 2).to("cuda"), feats.cuda()))
    assert torch.equal(a, b) and torch.equal(a, c)


def test_train_seg_main_trains_two_iterations_and_resumes_the_third_exactly(tmp_path, monkeypatch):
    """``--synthetic 2 --batch_size 2``: one iteration per epoch.  Run A: three epochs in one go.  Run B: two epochs, then a new
    fresh start resumed from B's files for the third."""
    from csn_amd import SegTrainer, train_seg
    losses = []
    inner = SegTrainer.train_epoch

    def recording(self):
        out = inner(self)
        assert self.iters_per_epoch == 1
        losses.append(out[0])
        return out
    monkeypatch.setattr(SegTrainer, "train_epoch", recording)
    common = ["--synthetic", "2", "--batch_size", "2", "--model", "Res16UNet14A", "--scheduler", "PolyLR", "--lr", "0.05", "--max_iter", "100"]
    assert train_seg.main(common + ["--max_epoch", "3", "--log_dir", str(tmp_path / "a")]) == 0
    a, losses[:] = list(losses), []
    assert train_seg.main(common + ["--max_epoch", "2", "--log_dir", str(tmp_path / "b")]) == 0
    state = torch.load(str(tmp_path / "b" / "weights.pth"))
    assert state["arch"] == "Res16UNet14A" and state["iteration"] == 3 and "final.weight" in state["state_dict"]
    assert train_seg.main(common + ["--max_epoch", "3", "--log_dir", str(tmp_path / "b"), "--resume", str(tmp_path / "b")]) == 0
    print(f"[unet] train_seg Res16UNet14A losses {a} | resumed {losses}")
    assert len(a) == 3 and all(np.isfinite(v) for v in a) and losses == a
