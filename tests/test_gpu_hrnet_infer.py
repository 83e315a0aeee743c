"""GPU parity of the inference backbone (csn_amd/minkowski_hrnet.py ``sparse_conv_bn_act``, ``HRNetBackbone`` under
``tuning.override(eval_epilogue=True)``, ``HRNetSeg``; the BN instances of csn_amd/csrc/sparse_conv.hip; include/csn_hip.h section 19),
in math modes 0 and 1, one case also on the single-product instances (modes 2 / 3 under ``csn_set_thread_rows16(1)``).

Single calls.  The point sets, convolution cases and pinned column blocks of tests/test_gpu_hrnet.py; per case: with and without a
residual, the residual aliasing ``y``, ReLU on and off, natural pitches and ``x`` / ``r`` / ``y`` as column blocks of wider
canary-filled buffers.  Reference: ``z32`` from ``csn_sparse_conv_fwd_f32`` on the same inputs in the same mode (the product's own
error is held by the existing tests), then ``act(z32 s + t + r)`` in float64 from the fp32 vectors.  Bound, elementwise:
``|y - ref| <= 2^-20 (|z32 s| + |beta| + |mean s| + |r|)`` — eight fp32 roundings of 2^-24 each (var + eps, sqrt, the division; mean
s, beta - mean s; the multiply-add; the residual add; and one to spare), times two; absolute, so a ReLU sign flip next to zero is
inside it.  Canaries intact; two calls give equal bits.

Backbone, 2S and 3S in eval under ``no_grad`` on the 300-voxel set and the set with two coarsest rows: every ``trace`` entry and the
output against ``hrnet_ref.backbone(training=False)`` in float64.  The yardstick is the switch-off path (the arithmetic the project
had) on the same case in the same mode: ITS error against float64 is measured, and the new path may have at most the larger of
1e-4 and twice that — the convention of tests/test_gpu_hrnet.py, for the maximum over the trace entries and for the output.  The
launches are counted: one ``csn_sparse_conv_bn_act_fwd_f32`` per convolution and nothing else of sections 14 / 15.  With autograd
enabled, in training mode or with ``fused=False`` the switch is ignored: bit-equal to switch off.

Models.  ``HRNetSeg3S`` training forward + backward bit-equal to the hand composition ``HRNetBackbone`` -> ``BackboneFC`` ->
``F.linear``; eval logits with the switch on against float64, bounded by the switch-off path as above; ``HRNetSimCSN3S`` eval logits
with one key batch, switch on against switch off, within the larger of 1e-4 and twice the switch-off logits' measured distance
from the same model run in math mode 0 (the only reference a head with attention has here; in mode 0 itself that distance is 0 and
the bound is 1e-4).

Measured on MI355X, maxima over the cases (fp32 / bf16x3; every test prints its own): see DESIGN.md "Inference backbone"."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R
from tests.test_gpu_hrnet import CANARY, CONVS, NB_CASES, NETS, SETS, _backbone_inputs, _batch, backbone_reference

pytestmark = pytest.mark.gpu

N_CONVS = {"2S": 22, "3S": 47}


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(params=[0, 1], ids=["fp32", "bf16x3"])
def math_mode(request, L):
    L.check(L.lib().csn_set_math_mode(request.param))
    yield request.param
    L.lib().csn_set_math_mode(1)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------
# single calls
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(mode, name, c_in, c_out, k):
    """Kernel map (CPU) and float32 CPU tensors of one convolution case; shared, never modified."""
    from csn_amd.minkowski_conv import build_kernel_map
    pts = torch.tensor(SETS[name]())
    if mode == "s1":
        m = build_kernel_map(pts, kernel_size=k)
    else:
        m = build_kernel_map(pts, kernel_size=3, stride=2)
        m = m if mode == "s2" else m.transpose()
    t = R.tensors(len(name) + c_in + 3 * c_out + k, m.n_in, m.n_out, m.KV, c_in, c_out)
    g = torch.Generator().manual_seed(11 * c_out + c_in + k)
    r = lambda *s: torch.randn(*s, generator=g)
    vec = {"gamma": 1 + 0.2 * r(c_out), "beta": 0.3 * r(c_out), "mean": 0.1 * r(c_out), "var": 1 + 0.1 * r(c_out).abs()}
    return m, t["x"], t["w"], vec, r(m.n_out, c_out)


def _block(t, wide, fill):
    """(n, C) CPU tensor -> (device view, its buffer or None); ``wide``: columns [8, 8 + C) of an (n, C + 20) buffer of ``fill``."""
    if not wide:
        return t.cuda().contiguous(), None
    n, C = t.shape
    buf = torch.full((n, C + 20), fill, dtype=torch.float32, device="cuda")
    buf[:, 8:8 + C] = t.cuda()
    return buf[:, 8:8 + C], buf


def _intact(buf, C, fill):
    return buf is None or (bool((buf[:, :8] == fill).all()) and bool((buf[:, 8 + C:] == fill).all()))


def _single_calls(L, case):
    """Every variant of one case; returns the worst ratio error / bound."""
    lib = L.lib()
    m, x_c, w_c, vec, r_c = case
    m = m.to("cuda")
    KV, c_in, c_out = w_c.shape
    n_in, n_out = m.n_in, m.n_out
    w = w_c.cuda().contiguous()
    v = {q: t.cuda() for q, t in vec.items()}
    x0 = x_c.cuda().contiguous()
    z32 = torch.empty(n_out, c_out, device="cuda")
    L.check(lib.csn_sparse_conv_fwd_f32(_ptr(x0), c_in, n_in, _ptr(m.fwd), n_out, KV, c_in, c_out, _ptr(w), None, _ptr(z32), c_out, _st()),
            "fwd")
    s = v["gamma"].double() / (v["var"].double() + H.EPS).sqrt()
    zs = z32.double() * s
    t = v["beta"].double() - v["mean"].double() * s
    base = zs.abs() + v["beta"].double().abs() + (v["mean"].double() * s).abs()
    worst = 0.0
    for wide in (False, True):
        x, _ = _block(x_c, wide, 1e30)
        for res in ("none", "own", "alias"):
            for relu in (True, False):
                r, _ = _block(r_c, wide, 1e30) if res == "own" else (None, None)
                y, ybuf = _block(r_c if res == "alias" else torch.full((n_out, c_out), CANARY), wide, CANARY)
                if res == "alias":
                    r = y
                outs = []
                for rep in range(2 if (res == "own" and relu) else 1):
                    if rep:
                        y, ybuf = _block(torch.full((n_out, c_out), CANARY), wide, CANARY)
                    L.check(lib.csn_sparse_conv_bn_act_fwd_f32(
                        _ptr(x), x.stride(0), n_in, _ptr(m.fwd), n_out, KV, c_in, c_out, _ptr(w), _ptr(v["gamma"]), _ptr(v["beta"]),
                        _ptr(v["mean"]), _ptr(v["var"]), H.EPS, _ptr(r), r.stride(0) if r is not None else 0, int(relu), _ptr(y),
                        y.stride(0), _st()), "bn_act fwd")
                    assert _intact(ybuf, c_out, CANARY), (wide, res, relu)
                    outs.append(y)
                if len(outs) == 2:
                    assert torch.equal(outs[0], outs[1]), "two calls differ"
                ref = zs + t + (r_c.cuda().double() if res != "none" else 0.0)
                if relu:
                    ref = ref.clamp_min(0)
                bound = 2.0 ** -20 * (base + (r_c.cuda().double().abs() if res != "none" else 0.0))
                ratio = ((y.double() - ref).abs() / bound).max().item()
                assert ratio <= 1.0, (wide, res, relu, ratio)
                worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", list(SETS))
def test_single_calls(L, math_mode, name):
    worst = 0.0
    for mode, c_in, c_out, k in CONVS:
        worst = max(worst, _single_calls(L, _case(mode, name, c_in, c_out, k)))
    print(f"[hrnet-infer] single calls {name} mode {math_mode}: worst error / bound {worst:.2f}")


def test_single_calls_with_pinned_column_blocks(L, math_mode):
    lib = L.lib()
    worst = 0.0
    try:
        for c_in, c_out, nb in NB_CASES:
            assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) >= 0
            worst = max(worst, _single_calls(L, _case("s1", "rand1031", c_in, c_out, 3)))
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    print(f"[hrnet-infer] pinned column blocks mode {math_mode}: worst error / bound {worst:.2f}")


@pytest.mark.parametrize("mode", [2, 3], ids=["bf16", "fp16"])
def test_single_calls_on_the_single_product_instances(L, mode):
    from csn_amd import functional as CF
    with CF.math_mode(mode), CF.rows16(True):
        assert L.lib().csn_get_thread_rows16() == 1
        worst = max(_single_calls(L, _case("s1", "rand129", 128, 128, 3)), _single_calls(L, _case("s2", "rand1031", 64, 128, 3)))
    print(f"[hrnet-infer] single product mode {mode}: worst error / bound {worst:.2f}")


def test_python_call_takes_pitched_views_and_pads_the_stem(L, math_mode):
    from csn_amd import sparse_conv_bn_act
    from csn_amd.minkowski_hrnet import _pitched
    m, x_c, w_c, vec, r_c = _case("s1", "rand129", 64, 64, 3)
    m = m.to("cuda")
    norm = torch.nn.BatchNorm1d(64).cuda().eval()
    with torch.no_grad():
        norm.weight.copy_(vec["gamma"]); norm.bias.copy_(vec["beta"]); norm.running_mean.copy_(vec["mean"]); norm.running_var.copy_(vec["var"])
    w = torch.nn.Parameter(w_c.cuda())
    x, _ = _block(x_c, True, 1e30)
    r, _ = _block(r_c, True, 1e30)
    assert _pitched(x) and not x.is_contiguous()
    plain = sparse_conv_bn_act(x_c.cuda(), w, m, norm, r_c.cuda(), True)
    assert plain.grad_fn is None and not plain.requires_grad and plain.shape == (m.n_out, 64)
    wide = torch.full((m.n_out, 160), CANARY, device="cuda")
    out = wide[:, 32:96]
    got = sparse_conv_bn_act(x, w, m, norm, r, True, out=out)
    assert got is out and torch.equal(out, plain) and bool((wide[:, :32] == CANARY).all()) and bool((wide[:, 96:] == CANARY).all())
    # a sum that accumulates in place: out = relu(conv s + t + out)
    acc = wide[:, 96:160]
    acc.copy_(r_c.cuda())
    sparse_conv_bn_act(x, w, m, norm, acc, True, out=acc)
    assert torch.equal(acc, plain) and torch.equal(out, plain) and bool((wide[:, :32] == CANARY).all())
    # views the kernels cannot take are made contiguous (x, residual) or refused (out)
    odd = torch.zeros(m.n_out, 67, device="cuda")[:, 1:65]
    odd.copy_(r_c.cuda())
    assert not _pitched(odd) and torch.equal(sparse_conv_bn_act(x, w, m, norm, odd, True), plain)
    with pytest.raises(ValueError, match="out"):
        sparse_conv_bn_act(x, w, m, norm, None, True, out=odd)
    # the stem: 3 colours zero-padded to 32
    ms, xs, ws, vs, _ = _case("s1", "rand33", 32, 32, 5)
    ms = ms.to("cuda")
    n32 = torch.nn.BatchNorm1d(32).cuda().eval()
    with torch.no_grad():
        n32.running_mean.copy_(vs["mean"]); n32.running_var.copy_(vs["var"])
    x3, w3 = xs[:, :3].cuda(), ws[:, :3].cuda()
    y3 = sparse_conv_bn_act(x3, w3, ms, n32, relu=False)
    full = sparse_conv_bn_act(F.pad(x3, (0, 29)), F.pad(w3, (0, 0, 0, 29)), ms, n32, relu=False)
    assert torch.equal(y3, full) and float(y3.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------
# the backbone
# ------------------------------------------------------------------------------------------------------
def _count_calls(L, fn):
    calls = {}

    def hook(name, phase):
        if phase == "begin":
            calls[name] = calls.get(name, 0) + 1
    L.set_call_hook(hook)
    try:
        out = fn()
    finally:
        L.set_call_hook(None)
    return out, calls


def _backbone(net, fused=True, training=False):
    from csn_amd import HRNetBackbone
    S, ff = NETS[net]
    bb = HRNetBackbone(3, S, ff, fused=fused).cuda().train(training)
    bb.load_state_dict(H.params(S, ff))
    return bb


def _pyramid(net, case):
    from csn_amd import build_pyramid
    pts, _, feats, _ = _backbone_inputs(net, case)
    return build_pyramid(torch.tensor(pts), NETS[net][0]).to("cuda"), feats.cuda()


def _errors(rows, trace, ref_rows, pre):
    assert sorted(trace) == sorted(pre)
    return {"y": (rows.cpu().double() - ref_rows).abs().max().item(),
            "trace": max((trace[k].cpu().double() - pre[k].clamp_min(0)).abs().max().item() for k in pre)}


@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_against_float64(L, math_mode, net, case):
    from csn_amd import tuning
    bb = _backbone(net)
    pyr, feats = _pyramid(net, case)
    ref_rows, pre, _ = backbone_reference(net, case, False)
    with torch.no_grad():
        t_off, t_on = {}, {}
        (rows_off, c_off) = _count_calls(L, lambda: bb(feats, pyr, t_off))
        with tuning.override(eval_epilogue=True):
            (rows_on, c_on) = _count_calls(L, lambda: bb(feats, pyr, t_on))
            again = bb(feats, pyr)
    base, got = _errors(rows_off, t_off, ref_rows, pre), _errors(rows_on, t_on, ref_rows, pre)
    print(f"[hrnet-infer] backbone {net} {case} mode {math_mode}: one launch y {got['y']:.1e} trace {got['trace']:.1e} | "
          f"two launches y {base['y']:.1e} trace {base['trace']:.1e}")
    assert c_on == {"csn_sparse_conv_bn_act_fwd_f32": N_CONVS[net]}, c_on
    assert "csn_sparse_conv_bn_act_fwd_f32" not in c_off and c_off["csn_sparse_conv_fwd_f32"] == N_CONVS[net]
    assert rows_on.grad_fn is None and rows_on.is_contiguous() and rows_on.shape == rows_off.shape
    assert torch.equal(rows_on, again)
    # the traced maps of the column blocks ARE the result's columns
    S, ff = NETS[net]
    assert torch.equal(t_on["bn0s1"], rows_on[:, :32]) and torch.equal(t_on[f"stages.{S - 1}.0.2.norm2"], rows_on[:, 32:32 + 32 * ff])
    assert torch.equal(t_on[f"final_transitions.{S - 2}.{3 * (S - 2) + 1}"], rows_on[:, -32 * ff * 2 ** (S - 1):])
    for q in ("y", "trace"):
        assert got[q] <= max(1e-4, 2 * base[q]), (q, got[q], base[q])


def test_backbone_falls_back_to_cat_past_the_window(L, monkeypatch):
    from csn_amd import minkowski_hrnet as MH
    from csn_amd import tuning
    bb = _backbone("2S")
    pyr, feats = _pyramid("2S", "rand300")
    with torch.no_grad(), tuning.override(eval_epilogue=True):
        whole = bb(feats, pyr)
        monkeypatch.setattr(MH, "_WINDOW", 300 * bb.out_channels * 4 - 1)
        parts, calls = _count_calls(L, lambda: bb(feats, pyr))
    assert calls == {"csn_sparse_conv_bn_act_fwd_f32": N_CONVS["2S"]} and torch.equal(parts, whole)


@pytest.mark.parametrize("how", ["grad_enabled", "training", "unfused"])
def test_the_switch_is_ignored_outside_inference(L, math_mode, how):
    from csn_amd import tuning
    net = "2S"
    pyr, feats = _pyramid(net, "rand300")
    outs = []
    for on in (False, True):
        bb = _backbone(net, fused=how != "unfused", training=how == "training")
        with torch.set_grad_enabled(how == "grad_enabled"), tuning.override(eval_epilogue=on):
            rows, calls = _count_calls(L, lambda: bb(feats, pyr))
        assert "csn_sparse_conv_bn_act_fwd_f32" not in calls
        outs.append((rows.detach(), bb.bn0s1.running_mean.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert (how == "grad_enabled") == (rows.grad_fn is not None)


# ------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------
def _seg_state(seed=3):
    """Backbone parameters of ``hrnet_ref.params`` and seeded ``final`` layers, as ``HRNetSeg3S(3, 6)``'s state dict (float32 CPU)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {f"backbone.{k}": v for k, v in H.params(3, 2).items()}
    sd.update({"final.0.weight": r(256, 480) / 480 ** 0.5, "final.0.bias": 0.1 * r(256), "final.1.weight": 1 + 0.2 * r(256),
               "final.1.bias": 0.3 * r(256), "final.1.running_mean": 0.1 * r(256), "final.1.running_var": 1 + 0.1 * r(256).abs(),
               "final.1.num_batches_tracked": torch.zeros((), dtype=torch.long), "final.3.weight": r(6, 256) / 16, "final.3.bias": 0.1 * r(6)})
    return sd


def test_seg3s_training_is_the_hand_composition(L, math_mode):
    from csn_amd import HRNetBackbone, HRNetSeg3S
    from csn_amd.minkowski_csn import BackboneFC
    sd = _seg_state()
    pyr, feats = _pyramid("3S", "rand300")
    dy = torch.randn(feats.shape[0], 6, generator=torch.Generator().manual_seed(9)).cuda()
    model = HRNetSeg3S(3, 6).cuda().train()
    model.load_state_dict(sd)
    x1 = feats.clone().requires_grad_(True)
    logits = model((pyr, x1))
    logits.backward(dy)
    bb, fc = HRNetBackbone(3, 3, 2).cuda().train(), BackboneFC(480, 256).cuda().train()
    bb.load_state_dict(H.params(3, 2))
    fc.load_state_dict({k[len("final."):]: v for k, v in sd.items() if k.startswith(("final.0", "final.1"))})
    w3, b3 = sd["final.3.weight"].cuda().requires_grad_(True), sd["final.3.bias"].cuda().requires_grad_(True)
    x2 = feats.clone().requires_grad_(True)
    want = F.linear(fc(bb(x2, pyr)), w3, b3)
    want.backward(dy)
    assert logits.shape == (feats.shape[0], 6) and torch.equal(logits, want) and torch.equal(x1.grad, x2.grad)
    grads = {k: v.grad for k, v in model.named_parameters()}
    ref = {**{f"backbone.{k}": v.grad for k, v in bb.named_parameters()}, **{f"final.{k}": v.grad for k, v in fc.named_parameters()},
           "final.3.weight": w3.grad, "final.3.bias": b3.grad}
    assert sorted(grads) == sorted(ref)
    for k, v in grads.items():
        assert v is not None and torch.equal(v, ref[k]), k
    assert int(model.final[1].num_batches_tracked) == 1 and torch.equal(model.final[1].running_mean, fc[1].running_mean)
    # bare coordinates build the same pyramid
    model.eval()
    with torch.no_grad():
        pts = torch.tensor(_backbone_inputs("3S", "rand300")[0])
        assert torch.equal(model((pts, feats)), model((pyr, feats)))


def test_seg3s_eval_against_float64(L, math_mode):
    from csn_amd import HRNetSeg3S, tuning
    sd = _seg_state()
    pyr, feats = _pyramid("3S", "rand300")
    rows, _, _ = backbone_reference("3S", "rand300", False)
    d = {k: v.double() for k, v in sd.items() if k.startswith("final.") and v.is_floating_point()}
    h = rows @ d["final.0.weight"].t() + d["final.0.bias"]
    h = ((h - d["final.1.running_mean"]) / (d["final.1.running_var"] + 1e-5).sqrt() * d["final.1.weight"] + d["final.1.bias"]).clamp_min(0)
    ref = h @ d["final.3.weight"].t() + d["final.3.bias"]
    model = HRNetSeg3S(3, 6).cuda().eval()
    model.load_state_dict(sd)
    with torch.no_grad():
        off = model((pyr, feats))
        with tuning.override(eval_epilogue=True):
            on, calls = _count_calls(L, lambda: model((pyr, feats)))
    base, got = (off.cpu().double() - ref).abs().max().item(), (on.cpu().double() - ref).abs().max().item()
    print(f"[hrnet-infer] HRNetSeg3S eval mode {math_mode}: one launch {got:.1e} | two launches {base:.1e}")
    assert calls.get("csn_sparse_conv_bn_act_fwd_f32") == 47 and calls.get("csn_rows_fc_fwd_f32") == 1
    assert got <= max(1e-4, 2 * base), (got, base)


def test_simcsn3s_eval_with_the_switch(L, math_mode):
    from csn_amd import HRNetSimCSN3S, tuning
    from csn_amd import functional as CF
    torch.manual_seed(4)
    model = HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().eval()
    model.backbone.load_state_dict(H.params(3, 2))                         # (a fresh BatchNorm is s = 1 / sqrt(1 + eps), t = 0)
    q, keys = _batch(0), [_batch(1)]
    with torch.no_grad():
        off = model(q, keys)
        with CF.math_mode(0):
            exact = model(q, keys)
        with tuning.override(eval_epilogue=True):
            on, calls = _count_calls(L, lambda: model(q, keys))
    base, got = (off - exact).abs().max().item(), (on - off).abs().max().item()
    print(f"[hrnet-infer] HRNetSimCSN3S eval K=1 mode {math_mode}: switch on vs off {got:.1e} | off vs math mode 0 {base:.1e}")
    assert calls.get("csn_sparse_conv_bn_act_fwd_f32") == 2 * 47 and "csn_rows_bn_act_fwd_f32" not in calls
    assert got <= max(1e-4, 2 * base), (got, base)
