"""GPU parity of the Res16UNets' inference graph (csn_amd/minkowski_unet.py ``octant_conv_bn_act``, ``UNetBasicBlock.infer``,
``Res16UNetBase._forward_infer`` under ``tuning.override(eval_epilogue=True)``; the BN instances of csn_amd/csrc/octant_conv.hip;
include/csn_hip.h section 23), in math modes 0 and 1.

Single calls, down and up.  The point sets, width lists and pinned column blocks of tests/test_gpu_octant.py (``SETS``, ``box128``
and ``box127_129``, ``WIDTHS``, ``NB_CASES`` on 1031 rows); per case: with and without a residual, the residual aliasing ``y``, ReLU
on and off, natural pitches and ``x`` / ``r`` / ``y`` as column blocks of wider canary-filled buffers.  Reference: ``z32`` from
``csn_octant_down_fwd_f32`` / ``csn_octant_up_fwd_f32`` on the same inputs in the same mode (the product's own error is held by
tests/test_gpu_octant.py), then ``act(z32 s + t + r)`` in float64 from the fp32 vectors.  Bound, elementwise:
``|y - ref| <= 2^-20 (|z32 s| + |beta| + |mean s| + |r|)`` — the derived bound of tests/test_gpu_hrnet_infer.py: eight fp32
roundings of 2^-24 each, times two; absolute, so a ReLU sign flip next to zero is inside it.  Canaries intact; two calls give
equal bits; a coarse row without children gives ``act(t + r)``.

Networks, eval under ``no_grad`` with the switch on: ``Res16UNet14`` on 300 voxels (every decoder block a chain over two column
blocks), ``Res16UNet14A`` on 300 voxels (none) and ``Res16UNet34C`` on 1031 voxels (one): the logits and every ``trace`` entry
against ``unet_ref.network(training=False)`` in float64.  The yardstick is the switch-off path on the same case in the same mode:
ITS error against float64 is measured, and the new path may have at most the larger of 1e-4 and twice that (the rule of
tests/test_gpu_unet.py and tests/test_gpu_hrnet_infer.py), for the maximum over the trace entries and for the logits.  The library
calls are counted: one section 19 or section 23 call per convolution + norm, two per convolution that reads a concatenation wider
than 256 columns, none of sections 14, 15 and 21.  With autograd enabled, in training mode or with ``fused=False`` the switch is
ignored: bit-equal to switch off.  With ``_WINDOW`` patched small the graph keeps separate maps + ``torch.cat`` within the same bound.

Measured on MI355X (every test prints its own figures): see DESIGN.md "Inference U-Net"."""
import functools

import pytest
import torch

from tests import octant_ref as O
from tests import unet_ref as U
from tests.test_gpu_octant import CANARY, MORE_SETS, NB_CASES, SETS, WIDTHS, _geometry
from tests.test_gpu_unet import N_OUT, _inputs, reference

pytestmark = pytest.mark.gpu

EPS = 1e-5
SINGLE_SETS = list(SETS) + ["box128", "box127_129"]
assert all(n in MORE_SETS for n in ("box128", "box127_129"))
S19, S23 = "csn_sparse_conv_bn_act_fwd_f32", ("csn_octant_down_bn_act_fwd_f32", "csn_octant_up_bn_act_fwd_f32")
# sections 14, 15 and 21: the launches of the training graph
OLD = ("csn_sparse_conv_fwd_f32", "csn_sparse_conv_stats_fwd_f32", "csn_rows_bn_act_fwd_f32", "csn_octant_down_fwd_f32",
       "csn_octant_up_fwd_f32")


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
def _case(up, name, c_in, c_out):
    """Octant map (CPU) and float32 CPU tensors of one case; shared, never modified."""
    p, m = _geometry(name)
    n_in, n_out = (p.n_coarse, p.n_fine) if up else (p.n_fine, p.n_coarse)
    t = O.tensors(len(name) + c_in + 3 * c_out + int(up), n_in, n_out, c_in, c_out)
    g = torch.Generator().manual_seed(13 * c_out + c_in + int(up))
    r = lambda *s: torch.randn(*s, generator=g)
    vec = {"gamma": 1 + 0.2 * r(c_out), "beta": 0.3 * r(c_out), "mean": 0.1 * r(c_out), "var": 1 + 0.1 * r(c_out).abs()}
    return m, t["x"], t["w"], vec, r(n_out, c_out)


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


def _call(L, up, m, x, w, v, r, relu, y, plain=False):
    """The section 23 call, or (``plain``) the section 21 call without a bias, on device tensors."""
    lib = L.lib()
    _, c_in, c_out = w.shape
    head = ((_ptr(x), x.stride(0), m.n_coarse, _ptr(m.parent), _ptr(m.order), _ptr(m.seg), m.n_fine, c_in, c_out, _ptr(w)) if up else
            (_ptr(x), x.stride(0), m.n_fine, _ptr(m.children), m.n_coarse, c_in, c_out, _ptr(w)))
    if plain:
        fn = lib.csn_octant_up_fwd_f32 if up else lib.csn_octant_down_fwd_f32
        L.check(fn(*head, None, _ptr(y), y.stride(0), _st()), "octant fwd")
    else:
        fn = lib.csn_octant_up_bn_act_fwd_f32 if up else lib.csn_octant_down_bn_act_fwd_f32
        L.check(fn(*head, _ptr(v["gamma"]), _ptr(v["beta"]), _ptr(v["mean"]), _ptr(v["var"]), EPS, _ptr(r),
                   r.stride(0) if r is not None else 0, int(relu), _ptr(y), y.stride(0), _st()), "octant bn_act fwd")


def _single_calls(L, up, case):
    """Every variant of one case; returns the worst ratio error / bound."""
    m, x_c, w_c, vec, r_c = case
    m = m.to("cuda")
    _, c_in, c_out = w_c.shape
    n_out = m.n_fine if up else m.n_coarse
    w = w_c.cuda().contiguous()
    v = {q: t.cuda() for q, t in vec.items()}
    z32 = torch.empty(n_out, c_out, device="cuda")
    _call(L, up, m, x_c.cuda().contiguous(), w, v, None, False, z32, plain=True)
    s = v["gamma"].double() / (v["var"].double() + EPS).sqrt()
    zs = z32.double() * s
    t = v["beta"].double() - v["mean"].double() * s
    base = zs.abs() + v["beta"].double().abs() + (v["mean"].double() * s).abs()
    r64 = r_c.cuda().double()
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
                    _call(L, up, m, x, w, v, r, relu, y)
                    assert _intact(ybuf, c_out, CANARY), (wide, res, relu)
                    outs.append(y)
                if len(outs) == 2:
                    assert torch.equal(outs[0], outs[1]), "two calls differ"
                ref = zs + t + (r64 if res != "none" else 0.0)
                if relu:
                    ref = ref.clamp_min(0)
                bound = 2.0 ** -20 * (base + (r64.abs() if res != "none" else 0.0))
                ratio = ((y.double() - ref).abs() / bound).max().item()
                assert ratio <= 1.0, (up, wide, res, relu, ratio)
                worst = max(worst, ratio)
    return worst


DIRS = pytest.mark.parametrize("up", [False, True], ids=["down", "up"])


@DIRS
@pytest.mark.parametrize("name", SINGLE_SETS)
def test_single_calls(L, math_mode, name, up):
    worst = 0.0
    for c_in, c_out in WIDTHS:
        worst = max(worst, _single_calls(L, up, _case(up, name, c_in, c_out)))
    print(f"[unet-infer] single calls {'up' if up else 'down'} {name} mode {math_mode}: worst error / bound {worst:.2f}")


@DIRS
def test_single_calls_with_pinned_column_blocks(L, math_mode, up):
    lib = L.lib()
    worst = 0.0
    try:
        for c_in, c_out, nb in NB_CASES:
            assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) >= 0
            worst = max(worst, _single_calls(L, up, _case(up, "rand1031", c_in, c_out)))
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)
    print(f"[unet-infer] pinned column blocks {'up' if up else 'down'} mode {math_mode}: worst error / bound {worst:.2f}")


def test_a_coarse_row_without_children_gives_the_shift(L, math_mode):
    """The down launch on a map whose first coarse row has lost its children: ``y[0] = act(t + r[0])``."""
    m, x_c, w_c, vec, r_c = _case(False, "rand129", 64, 96)
    m = m.to("cuda")
    children = m.children.clone()
    children[:, 0] = -1
    v = {q: t.cuda() for q, t in vec.items()}
    x, w, r = x_c.cuda(), w_c.cuda().contiguous(), r_c.cuda().contiguous()
    s = v["gamma"].double() / (v["var"].double() + EPS).sqrt()
    t = v["beta"].double() - v["mean"].double() * s
    bound = 2.0 ** -20 * (v["beta"].double().abs() + (v["mean"].double() * s).abs() + r[0].double().abs())
    lib = L.lib()
    for relu in (True, False):
        y = torch.full((m.n_coarse, 96), CANARY, device="cuda")
        L.check(lib.csn_octant_down_bn_act_fwd_f32(_ptr(x), 64, m.n_fine, _ptr(children), m.n_coarse, 64, 96, _ptr(w), _ptr(v["gamma"]),
                                                   _ptr(v["beta"]), _ptr(v["mean"]), _ptr(v["var"]), EPS, _ptr(r), 96, int(relu), _ptr(y),
                                                   96, _st()), "down bn_act")
        want = t + r[0].double()
        want = want.clamp_min(0) if relu else want
        assert bool(((y[0].double() - want).abs() <= bound).all()) and bool((y != CANARY).all())


def test_python_call_takes_pitched_views(L, math_mode):
    from csn_amd import octant_conv_bn_act
    from csn_amd.minkowski_hrnet import _pitched
    for up in (False, True):
        m, x_c, w_c, vec, r_c = _case(up, "rand129", 64, 96)
        m = m.to("cuda")
        n_out = m.n_fine if up else m.n_coarse
        norm = torch.nn.BatchNorm1d(96).cuda().eval()
        with torch.no_grad():
            norm.weight.copy_(vec["gamma"]); norm.bias.copy_(vec["beta"]); norm.running_mean.copy_(vec["mean"]); norm.running_var.copy_(vec["var"])
        w = torch.nn.Parameter(w_c.cuda())
        x, _ = _block(x_c, True, 1e30)
        r, _ = _block(r_c, True, 1e30)
        assert _pitched(x) and not x.is_contiguous()
        plain = octant_conv_bn_act(x_c.cuda(), w, m, norm, up, r_c.cuda(), True)
        assert plain.grad_fn is None and not plain.requires_grad and plain.shape == (n_out, 96)
        wide = torch.full((n_out, 256), CANARY, device="cuda")
        out = wide[:, 32:128]
        got = octant_conv_bn_act(x, w, m, norm, up, r, True, out=out)
        assert got is out and torch.equal(out, plain) and bool((wide[:, :32] == CANARY).all()) and bool((wide[:, 128:] == CANARY).all())
        acc = wide[:, 128:224]
        acc.copy_(r_c.cuda())
        octant_conv_bn_act(x, w, m, norm, up, acc, True, out=acc)
        assert torch.equal(acc, plain) and torch.equal(out, plain) and bool((wide[:, 224:] == CANARY).all())
        odd = torch.zeros(n_out, 99, device="cuda")[:, 1:97]
        odd.copy_(r_c.cuda())
        assert not _pitched(odd) and torch.equal(octant_conv_bn_act(x, w, m, norm, up, odd, True), plain)
        with pytest.raises(ValueError, match="out"):
            octant_conv_bn_act(x, w, m, norm, up, None, True, out=odd)


# ------------------------------------------------------------------------------------------------------
# the networks
# ------------------------------------------------------------------------------------------------------
NETS = [("Res16UNet14", 300), ("Res16UNet14A", 300), ("Res16UNet34C", 1031)]
NET_IDS = [f"{a}-{n}" for a, n in NETS]


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


def _expected_calls(net):
    """(section 19 calls, section 23 calls) of one forward: a convolution that reads more than 256 columns counts twice."""
    planes, layers = U.NETS[net]
    n19, inplanes = 1, U.INIT_DIM
    skips = (planes[2], planes[1], planes[0], U.INIT_DIM)
    for n in range(1, 9):
        c = planes[n - 1]
        ci = inplanes if n <= 4 else planes[n - 1] + skips[n - 5]
        for i in range(layers[n - 1]):
            first = ci if i == 0 else c
            reads = 2 if first > 256 else 1
            n19 += reads + 1 + (reads if first != c else 0)
        inplanes = c
    return n19, 8


def _model(net, fused=True, training=False):
    import csn_amd
    model = getattr(csn_amd, net)(3, N_OUT, fused=fused).cuda().train(training)
    model.load_state_dict(U.params(net))
    return model


def _pyramid(n):
    import csn_amd
    pts, _, feats, _ = _inputs(n)
    return csn_amd.build_unet_pyramid(torch.tensor(pts)).to("cuda"), feats.cuda()


def _errors(y, trace, net, n):
    ref_y, pre, _ = reference(net, n, False)
    assert sorted(trace) == sorted(pre)
    return {"y": (y.cpu().double() - ref_y).abs().max().item(),
            "trace": max((trace[k].cpu().double() - pre[k].clamp_min(0)).abs().max().item() for k in pre)}


@pytest.mark.parametrize("net,n", NETS, ids=NET_IDS)
def test_network_against_float64(L, math_mode, net, n):
    from csn_amd import tuning
    model = _model(net)
    pyr, feats = _pyramid(n)
    with torch.no_grad():
        t_off, t_on = {}, {}
        y_off, c_off = _count_calls(L, lambda: model((pyr, feats), t_off))
        with tuning.override(eval_epilogue=True):
            y_on, c_on = _count_calls(L, lambda: model((pyr, feats), t_on))
            again = model((pyr, feats))
    base, got = _errors(y_off, t_off, net, n), _errors(y_on, t_on, net, n)
    print(f"[unet-infer] {net} n {n} mode {math_mode}: one launch y {got['y']:.1e} trace {got['trace']:.1e} | "
          f"training graph y {base['y']:.1e} trace {base['trace']:.1e} | calls {sum(c_on.values())} vs {sum(c_off.values())}")
    n19, n23 = _expected_calls(net)
    assert c_on == {S19: n19, S23[0]: n23 // 2, S23[1]: n23 // 2}, c_on
    assert not any(q in c_on for q in OLD) and S19 not in c_off and not any(q in c_off for q in S23)
    assert y_on.grad_fn is None and y_on.shape == y_off.shape and torch.equal(y_on, again)
    for q in ("y", "trace"):
        assert got[q] <= max(1e-4, 2 * base[q]), (q, got[q], base[q])


def test_expected_call_counts_are_the_networks():
    """The counting rule on the three networks: 14 has four wide decoder blocks (conv1 and downsample twice each), 14A none, 34C one."""
    assert [_expected_calls(net) for net, _ in NETS] == [(32, 8), (24, 8), (56, 8)]


@pytest.mark.parametrize("how", ["grad_enabled", "training", "unfused"])
def test_the_switch_is_ignored_outside_inference(L, math_mode, how):
    from csn_amd import tuning
    net, n = "Res16UNet14A", 300
    pyr, feats = _pyramid(n)
    outs = []
    for on in (False, True):
        model = _model(net, fused=how != "unfused", training=how == "training")
        with torch.set_grad_enabled(how == "grad_enabled"), tuning.override(eval_epilogue=on):
            y, calls = _count_calls(L, lambda: model((pyr, feats)))
        assert S19 not in calls and not any(q in calls for q in S23)
        outs.append((y.detach(), model.bn0.running_mean.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert (how == "grad_enabled") == (y.grad_fn is not None)


def test_network_falls_back_to_cat_past_the_window(L, math_mode, monkeypatch):
    from csn_amd import minkowski_hrnet as MH
    from csn_amd import tuning
    net, n = "Res16UNet14", 300
    model = _model(net)
    pyr, feats = _pyramid(n)
    with torch.no_grad():
        y_off = model((pyr, feats))
        with tuning.override(eval_epilogue=True):
            whole = model((pyr, feats))
            monkeypatch.setattr(MH, "_WINDOW", 1)                          # no level's buffer fits
            t_parts = {}
            parts, calls = _count_calls(L, lambda: model((pyr, feats), t_parts))
    n19, n23 = _expected_calls(net)
    assert calls == {S19: n19, S23[0]: n23 // 2, S23[1]: n23 // 2}
    assert torch.equal(parts, whole)                                       # the same launches on the same values
    ref_y = reference(net, n, False)[0]
    base, got = (y_off.cpu().double() - ref_y).abs().max().item(), _errors(parts, t_parts, net, n)["y"]
    assert got <= max(1e-4, 2 * base), (got, base)
