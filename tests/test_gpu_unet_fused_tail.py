"""GPU parity of the Res16UNets' training step under ``tuning.unet_fused_tail`` (csn_amd/minkowski_unet.py: the eight resolution
changes on ``octant_conv_stats`` + ``bn_act``, the two convolutions of a block wider than 256 columns on ``cat_conv_stats``) against
the float64 restatement tests/unet_ref.py: ``Res16UNet14`` (four wide blocks) and ``Res16UNet34C`` (one) on the 300-voxel case and
parameters of tests/test_gpu_unet.py, training mode, math modes 0 (fp32) and 1 (bf16x3).

Accuracy.  Logits, every parameter gradient (and the input's) and every running statistic against ``unet_ref.network`` in float64,
the gradients under the model's own ReLU masks (its trace), as tests/test_gpu_unet.py takes them.  The project's rule for whole
networks: with the switch, each quantity may err at most max(1e-4, 2 x the error of ``fused=False`` on the same case in the same
mode); both are measured here.  The float64 pre-activations of these cases lie within 1e-4 of zero for at most 0.1 % of their
elements (tests/test_cpu_unet_fused_tail.py asserts it on the reference alone), so a mask that flips there moves no figure by more
than that distance.

Launches, through ``_lib.set_call_hook``: with the switch a training forward calls the section-26 entry points eight times, section
21's forwards never and section 27's twice per wide block; with the switch off, in eval mode or with ``fused=False`` none of the new
names is called.  ``num_batches_tracked`` equals the unfused network's.

Measured on MI355X (every test prints its own), fused tail | unfused.  ``Res16UNet14`` fp32: y 1.3e-5 | 1.1e-5, gradients 5.8e-6 |
5.5e-6, running statistics 7.2e-8 | 1.4e-7; bf16x3: y 1.6e-4 | 1.7e-4, gradients 7.1e-5 | 7.8e-5, running statistics 7.8e-7 | 7.8e-7.
``Res16UNet34C`` fp32: y 2.4e-5 | 1.7e-5, gradients 1.1e-5 | 1.3e-5, running statistics 1.7e-7 | 2.1e-7; bf16x3: y 3.7e-4 | 2.6e-4,
gradients 1.6e-4 | 1.9e-4, running statistics 1.9e-6 | 1.9e-6."""
import collections

import pytest
import torch

from tests import unet_ref as U
from tests.test_gpu_unet import N_OUT, _errors, _inputs, _show

pytestmark = pytest.mark.gpu

N = 300
NETS = {"Res16UNet14": 4, "Res16UNet34C": 1}                     # the blocks that read more than 256 columns
NEW = ("csn_octant_down_stats_fwd_f32", "csn_octant_up_stats_fwd_f32", "csn_sparse_conv_cat_stats_fwd_f32")


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_math_mode(1)
    L.set_call_hook(None)


def _run(L, net, training, fused, tail, grad=True):
    """One forward (+ backward) of the model; returns (errors or None, forward call counts, state dict, logits)."""
    import csn_amd
    from csn_amd import tuning
    pts, _, feats, dy = _inputs(N)
    model = getattr(csn_amd, net)(3, N_OUT, fused=fused).cuda().train(training)
    model.load_state_dict(U.params(net))
    pyr = csn_amd.build_unet_pyramid(torch.tensor(pts)).to("cuda")
    x = feats.cuda().requires_grad_(training)
    trace, calls = {}, collections.Counter()
    L.set_call_hook(lambda name, phase: calls.update([name]) if phase == "begin" else None)
    try:
        with tuning.override(unet_fused_tail=tail), (torch.enable_grad() if training else torch.no_grad()):
            y = model((pyr, x), trace)
    finally:
        L.set_call_hook(None)
    sd = model.state_dict()
    if not (training and grad):
        return None, calls, sd, y.detach()
    with tuning.override(unet_fused_tail=tail):
        y.backward(dy.cuda())
    grads = {"feats": x.grad, **{k: v.grad for k, v in model.named_parameters()}}
    return _errors(net, N, True, y, grads, {k: v.cpu() > 0 for k, v in trace.items()}, sd), calls, sd, y.detach()


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("net", list(NETS))
def test_training_step_against_float64(L, net, mode):
    L.check(L.lib().csn_set_math_mode(mode))
    tail, calls, sd_t, _ = _run(L, net, True, True, True)
    plain, _, sd_p, _ = _run(L, net, True, False, False)
    print(f"[unet tail] {net} n {N} mode {mode}: " + " | ".join(_show(t, e) for t, e in (("fused tail", tail), ("unfused", plain))))
    for q in ("y", "grad", "running"):
        assert tail[q] <= max(1e-4, 2 * plain[q]), (q, tail[q], plain[q])
    # the launches of the forward
    assert calls["csn_octant_down_stats_fwd_f32"] == 4 and calls["csn_octant_up_stats_fwd_f32"] == 4
    assert calls["csn_octant_down_fwd_f32"] == 0 and calls["csn_octant_up_fwd_f32"] == 0
    assert calls["csn_sparse_conv_cat_stats_fwd_f32"] == 2 * NETS[net]
    # the norms have counted their batches as ATen's do
    tracked = [k for k in sd_p if k.endswith("num_batches_tracked")]
    assert tracked and all(int(sd_t[k]) == int(sd_p[k]) == 1 for k in tracked)


@pytest.mark.parametrize("net", list(NETS))
def test_the_switch_changes_nothing_where_it_does_not_apply(L, net):
    """Off, in eval mode or with ``fused=False``: none of the new entry points is called, and the logits are today's bits."""
    for training, fused in ((True, True), (False, True), (True, False), (False, False)):
        base = _run(L, net, training, fused, False, grad=False)
        assert not any(base[1][k] for k in NEW), (training, fused)
        if training and fused:
            continue                                                 # the one combination the switch acts on
        on = _run(L, net, training, fused, True, grad=False)
        assert not any(on[1][k] for k in NEW), (training, fused)
        assert torch.equal(on[3], base[3]), (training, fused)
        for k, v in base[2].items():
            assert torch.equal(on[2][k], v), k
