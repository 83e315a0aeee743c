"""GPU checks of ``tuning.train_maps16`` on the networks: ``HRNetBackbone`` 2S / 3S, ``HRNetSeg3S`` and ``HRNetSimCSN3S`` in training, math
mode "bf16" with ``rows_single_product``.

The contract is exactness.  The graph under the switch equals the single-product graph on fp32 maps with every stored bf16 map
rounded once.  The reference is COMPOSED here from the public calls as they stand without the switch: ``conv_stats``,
``bn_act(..., relu=False)``, a straight-through rounding node (forward ``v.to(bfloat16).float()``, backward the identity) and
``torch.relu`` — round(relu(v)) == relu(round(v)), and ``torch.relu`` masks on the rounded value as the new backward does.  One
training forward + backward from a random ``dy``: the result, every traced map (the stored bf16 widened), the gradient of every
parameter and of the input features and the running statistics are compared with ``torch.equal``; two runs give the same bits.

No saved tensor of the backward graph is an fp32 copy of a map that is stored as bf16 (the graph is walked through
``grad_fn.next_functions``), and the bf16 rows themselves are what the consuming convolution nodes saved.

Where the switch does nothing — math modes "fp16", "fp32" and "bf16x3", ``rows_single_product`` off, ``fused=False``, a
``GroupedPyramid`` and ``HRNetSimCSN3S`` under ``grouped_passes``, eval mode of the backbone or of one block, a Res16UNet's training
step — results, gradients and buffers are bit-equal to the switch being off."""
import copy
import types

import pytest
import torch

from tests import hrnet_ref as H
from tests.test_gpu_hrnet import NETS, _backbone_inputs, _batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        return v.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g


def composed_forward(self, feats, pyramid, trace=None):
    """``HRNetBackbone.forward`` in training, written out on the public section-15 calls, every map that the switch stores as bf16
    rounded once before its ReLU."""
    from csn_amd import bn_act, conv_stats
    trace = {} if trace is None else trace
    S = self.num_stages

    def term(conv, norm, x, kmap):
        norm.num_batches_tracked += 1
        z, mean, invstd = conv_stats(x, conv.kernel, kmap, norm.running_mean, norm.running_var, norm.eps, norm.momentum)
        return (z, mean, invstd, norm.weight, norm.bias)

    def act(name, terms, r=None, store16=True):
        v = bn_act(terms, r, relu=False, training=True)
        y = torch.relu(_Round.apply(v) if store16 else v)
        trace[name] = y.detach()
        return y

    out_init = act("bn0s1", [term(self.conv0s1, self.bn0s1, feats.float(), pyramid.stem)], store16=False)
    stage_input = [act("bn1s1", [term(self.conv1s1, self.bn1s1, out_init, pyramid.s1[0])])]
    for i in range(S):
        stage_output = []
        for j in range(i + 1):
            x = stage_input[j]
            for b, blk in enumerate(self.stages[i][j]):
                last = i == S - 1 and j == 0 and b == len(self.stages[i][j]) - 1
                n = f"stages.{i}.{j}.{b}."
                h = act(n + "norm1", [term(blk.conv1, blk.norm1, x, pyramid.s1[j])])
                x = act(n + "norm2", [term(blk.conv2, blk.norm2, h, pyramid.s1[j])], x, store16=not last)
            stage_output.append(x)
        if i == S - 1:
            break
        depth = i + 1
        stage_input = []
        for k in range(depth + 1):
            terms, res = [], None
            for j in range(depth):
                if j == k:
                    res = stage_output[j]
                    continue
                path, x, steps = self.exchange_blocks[i][j][k], stage_output[j], abs(k - j)
                for s in range(steps):
                    level = j + s if k > j else j - s
                    kmap = pyramid.down[level] if k > j else pyramid.up(level - 1)
                    t = term(path[3 * s], path[3 * s + 1], x, kmap)
                    if s + 1 < steps:
                        x = act(f"exchange_blocks.{i}.{j}.{k}.{3 * s + 1}", [t])
                    else:
                        terms.append(t)
            if terms:
                stage_input.append(act(f"sum.{i}.{k}", terms, res))
            else:
                trace[f"sum.{i}.{k}"] = res.detach()
                stage_input.append(res)
    outs = [out_init, stage_output[0]]
    for i in range(1, S):
        x, block = stage_output[i], self.final_transitions[i - 1]
        for s in range(i):
            x = act(f"final_transitions.{i - 1}.{3 * s + 1}", [term(block[3 * s], block[3 * s + 1], x, pyramid.up(i - s - 1))],
                    store16=s != i - 1)
        outs.append(x)
    return torch.cat(outs, dim=1)


FP32_MAPS = {"2S": {"bn0s1", "stages.1.0.2.norm2", "final_transitions.0.1"},
             "3S": {"bn0s1", "stages.2.0.2.norm2", "final_transitions.0.1", "final_transitions.1.4"}}


def _mode16():
    from csn_amd import functional as CF
    from csn_amd import tuning
    return CF.math_mode("bf16"), tuning.override(rows_single_product=True)


def _step(net, case, on, composed=False):
    """One training forward + backward of the backbone: (rows, trace, gradients, buffers, the result with its graph)."""
    from csn_amd import HRNetBackbone, build_pyramid, tuning
    S, ff = NETS[net]
    pts, _, feats, dy = _backbone_inputs(net, case)
    bb = HRNetBackbone(3, S, ff).cuda().train()
    bb.load_state_dict(H.params(S, ff))
    if composed:
        bb.forward = types.MethodType(composed_forward, bb)
    pyr = build_pyramid(torch.tensor(pts), S).to("cuda")
    x = feats.cuda().requires_grad_(True)
    trace = {}
    mode, single = _mode16()
    with mode, single, tuning.override(train_maps16=on):
        rows = bb(x, pyr, trace)
        rows.backward(dy.cuda(), retain_graph=True)
    grads = {"feats": x.grad, **{k: v.grad for k, v in bb.named_parameters()}}
    return rows, trace, grads, dict(bb.named_buffers())


@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_step_equals_the_composed_reference(L, net, case):
    rows, trace, grads, bufs = _step(net, case, True)
    want_rows, want_trace, want_grads, want_bufs = _step(net, case, False, composed=True)
    assert rows.dtype == torch.float32 and torch.equal(rows, want_rows)
    assert sorted(trace) == sorted(want_trace)
    for name, t in trace.items():
        assert t.dtype == (torch.float32 if name in FP32_MAPS[net] else torch.bfloat16), name
        assert not t.requires_grad and torch.equal(t.float(), want_trace[name]), name
    assert sorted(grads) == sorted(want_grads)
    for name, g in grads.items():
        assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), name
        assert torch.equal(g, want_grads[name]), (name, (g - want_grads[name]).abs().max().item())
    for name, b in bufs.items():
        assert torch.equal(b, want_bufs[name]), name
    # two identical runs give the same bits
    rows2, trace2, grads2, _ = _step(net, case, True)
    assert torch.equal(rows, rows2) and all(torch.equal(t, trace2[k]) for k, t in trace.items())
    assert all(torch.equal(g, grads2[k]) for k, g in grads.items())


def _saved_tensors(root):
    """(name of the node's class, saved tensor) over the whole backward graph of ``root``."""
    seen, stack, out = set(), [root.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        out += [(type(fn).__name__, t) for t in (getattr(fn, "saved_tensors", None) or ()) if isinstance(t, torch.Tensor)]
        stack += [f for f, _ in fn.next_functions]
    return out


@pytest.mark.parametrize("net", ["2S", "3S"])
def test_no_fp32_copy_of_a_bf16_map_is_saved(L, net):
    rows, trace, _, _ = _step(net, "rand300", True)
    saved = _saved_tensors(rows)
    stored = {k: t for k, t in trace.items() if t.dtype == torch.bfloat16}
    assert len(stored) == len(trace) - len(FP32_MAPS[net])
    # every stored map feeds a convolution: that CONSUMER (not only the bn_act that wrote the map and keeps it for its mask) saved
    # the bf16 rows themselves, and its first saved tensor — the gathered x — is bf16 at every such node
    conv_x = [t for node, t in saved if node == "_ConvStats16Backward" and t.dim() == 2]
    assert conv_x and all(t.dtype == torch.bfloat16 for t in conv_x)
    ptrs = {t.data_ptr() for t in conv_x}
    for name, t in stored.items():
        assert t.data_ptr() in ptrs, f"{name}: the consuming convolution did not save the bf16 rows"
        wide = t.float()
        for node, s in saved:
            assert not (s.dtype == torch.float32 and s.shape == wide.shape and torch.equal(s, wide)), f"{node} saved an fp32 copy of {name}"
    # ... while the fp32-map graph does save them (the walk sees what it should)
    rows0, trace0, _, _ = _step(net, "rand300", False)
    saved0 = _saved_tensors(rows0)
    assert any(node == "_ConvStatsBackward" and s.shape == trace0["bn1s1"].shape and torch.equal(s, trace0["bn1s1"]) for node, s in saved0)


def _inert(build, run):
    """``run(model)`` -> tensors, with the switch off and on: equal bits."""
    from csn_amd import tuning
    outs = []
    for on in (False, True):
        with tuning.override(train_maps16=on):
            outs.append(run(build()))
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("where", ["fp16", "fp32", "bf16x3", "bf16 without rows_single_product", "fused=False", "grouped", "eval",
                                   "a frozen block"])
def test_the_switch_does_nothing_elsewhere(L, where):
    from csn_amd import HRNetBackbone, build_pyramid, merge_batches, tuning
    from csn_amd import functional as CF
    S, ff = NETS["2S"]
    pts, _, feats, dy = _backbone_inputs("2S", "rand300")
    mode = {"fp16": "fp16", "fp32": "fp32", "bf16x3": "bf16x3"}.get(where, "bf16")

    def build():
        bb = HRNetBackbone(3, S, ff, fused=where != "fused=False").cuda().train(where != "eval")
        bb.load_state_dict(H.params(S, ff))
        if where == "a frozen block":                                       # its two norms run on their running statistics
            bb.stages[1][0][1].eval()
        return bb

    def run(bb):
        if where == "grouped":
            batches = [_batch(0), _batch(1)]                                # two batches of 300 voxels, rows sorted by shape
            pyr = merge_batches(batches, S).to("cuda")
            x = torch.cat([f for _, f in batches]).requires_grad_(True)
            out_grad = torch.cat([dy, dy]).cuda()
        else:
            pyr = build_pyramid(torch.tensor(pts), S).to("cuda")
            x, out_grad = feats.cuda().requires_grad_(True), dy.cuda()
        trace = {}
        with CF.math_mode(mode), tuning.override(rows_single_product=where != "bf16 without rows_single_product"):
            rows = bb(x, pyr, trace)
            rows.backward(out_grad)
        assert all(t.dtype == torch.float32 for t in trace.values())
        return [rows.detach(), x.grad] + [p.grad for p in bb.parameters()] + [b for b in bb.buffers()]

    _inert(build, run)


def test_the_res16unets_ignore_the_switch(L):
    """One training step of a Res16UNet in math mode "bf16" with ``rows_single_product``, the ATen tail and the fused tail: logits,
    gradients and buffers with the switch on are the bits of the switch off."""
    from csn_amd import functional as CF
    from csn_amd import tuning
    from tests.test_gpu_unet_infer import _model, _pyramid as _unet_pyramid
    pyr, feats = _unet_pyramid(300)

    def run(model):
        x = feats.clone().requires_grad_(True)
        y = model((pyr, x))
        y.square().mean().backward()
        return [y.detach(), x.grad] + [p.grad for p in model.parameters()] + [b for b in model.buffers()]

    for tail in (False, True):
        with CF.math_mode("bf16"), tuning.override(rows_single_product=True, unet_fused_tail=tail):
            _inert(lambda: _model("Res16UNet14", training=True), run)


def test_simcsn3s_under_grouped_passes_ignores_the_switch(L):
    """``HRNetSimCSN3S.forward(queries, keys)`` with ``tuning.grouped_passes``: the K + 1 batches run as one pass on a merged pyramid,
    which has no bf16-map form — logits, gradients and buffers with the switch on are the bits of the switch off (both steps seeded
    alike: the head's attention dropout draws its seeds from torch's generator)."""
    from csn_amd import HRNetSimCSN3S, tuning
    from csn_amd import functional as CF

    def build():
        torch.manual_seed(5)
        return HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().train()

    def run(model):
        torch.manual_seed(11)
        logits = model(_batch(0), [_batch(1)])
        logits.square().mean().backward()
        return [logits.detach()] + [p.grad for p in model.parameters() if p.grad is not None] + [b for b in model.buffers()]

    with CF.math_mode("bf16"), tuning.override(rows_single_product=True, grouped_passes=True):
        _inert(build, run)


def _head_step(model, batch_args):
    """One training step of ``model`` under the switch and of a copy on the composed backbone: per model the logits, the rows its
    backbone handed to the head (one entry per pass), the parameters and the buffers."""
    from csn_amd import tuning
    ref = copy.deepcopy(model)
    ref.backbone.forward = types.MethodType(composed_forward, ref.backbone)
    outs = []
    for m, on in ((model, True), (ref, False)):
        rows = []
        hook = m.backbone.register_forward_hook(lambda mod, args, out, rows=rows: rows.append(out.detach().clone()))
        mode, single = _mode16()
        # the head's attention dropout (p = 0.1, as the reference's) draws its seeds from torch's generator: the same for both steps
        torch.manual_seed(11)
        with mode, single, tuning.override(train_maps16=on):
            logits = m(*batch_args)
            logits.square().mean().backward()
        hook.remove()
        outs.append((logits.detach(), rows, dict(m.named_parameters()), dict(m.named_buffers())))
    return outs


def _assert_logits_and_gradients_equal(outs):
    (a, _, pa, ba), (b, _, pb, bb_) = outs
    assert torch.equal(a, b), (a - b).abs().max().item()
    for name, p in pa.items():
        if p.grad is None:
            assert pb[name].grad is None, name
            continue
        assert p.grad.dtype == torch.float32 and torch.equal(p.grad, pb[name].grad), name
    for name, t in ba.items():
        assert torch.equal(t, bb_[name]), name


def test_seg3s_through_its_public_forward(L):
    from csn_amd import HRNetSeg3S
    torch.manual_seed(4)
    outs = _head_step(HRNetSeg3S(3, 6).cuda().train(), (_batch(0),))
    assert len(outs[0][1]) == 1 and torch.equal(outs[0][1][0], outs[1][1][0])
    _assert_logits_and_gradients_equal(outs)


def _simcsn_step():
    from csn_amd import HRNetSimCSN3S
    torch.manual_seed(5)
    return _head_step(HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().train(), (_batch(0), [_batch(1)]))


def test_simcsn3s_backbone_passes_through_its_public_forward(L):
    """K = 1 on separate passes: the rows the backbone hands to the head for the queries and for the key batch, and the backbone's
    running statistics after both passes, equal the composed reference's bit for bit."""
    (_, rows, _, bufs), (_, want_rows, _, want_bufs) = _simcsn_step()
    assert len(rows) == 2 and all(torch.equal(a, b) for a, b in zip(rows, want_rows))
    for name, t in bufs.items():
        if name.startswith("backbone."):
            assert torch.equal(t, want_bufs[name]), name


def test_simcsn3s_logits_and_gradients_through_its_public_forward(L):
    """The logits and every parameter's gradient (the head's included) against the composed reference, bit for bit."""
    _assert_logits_and_gradients_equal(_simcsn_step())
