"""GPU checks of the 16-bit inference maps (include/csn_hip.h section 24, csn_amd/csrc/sparse_conv_maps16.hip,
``sparse_conv_bn_act`` on 16-bit tensors, ``HRNetBackbone`` under ``tuning.override(infer_maps16=True)``), in math modes 2 (bf16) and
3 (fp16) with the single-product instances selected.

The contract is exactness, so nothing here but the float64 comparison has a tolerance: a 16-bit map changes where a value is rounded,
not which product is formed.  Given the same representable inputs, a launch on 16-bit maps is bit-identical to
``csn_sparse_conv_bn_act_fwd_f32`` under ``csn_set_thread_rows16(1)`` in the same mode, with its fp32 output rounded once (torch's
cast: nearest even) when the output map is 16-bit.  Inputs go through ``rows16_ref.no_subnormals``.

Single calls.  Convolution cases x point sets of tests/test_gpu_hrnet.py that reach every path at the smallest size: every NB
instance (``NB_CASES`` pinned), a partial last row tile (1031 = 8 * 128 + 7), dropped offsets (``two``), the k = 5 stem width, both
strided maps.  All eight ``(x16, r16, y16)`` combinations x residual none / own / aliasing ``y`` (where the types allow) x ReLU on /
off x natural pitches and column blocks [8, 8 + C) of (n, C + 24) canary-filled buffers of the map's own dtype: ``torch.equal`` with
the section-19 result (rounded for a 16-bit ``y``), canaries intact, two calls equal, all flags 0 equal to section 19.

Backbone.  2S and 3S on ``rand300`` and ``coarse2`` in eval under ``no_grad`` with ``eval_epilogue + rows_single_product +
infer_maps16`` against an EMULATION: the same model with ``infer_maps16=False`` and ``sparse_conv_bn_act`` wrapped so that every
written map that is not a column block of the result is rounded once, in place (``.to(dtype).float()``).  Output and every trace entry
are equal bit for bit; the launches are counted (one ``csn_sparse_conv_bn_act_fwd_m16`` per convolution, nothing of sections 14 / 15 /
19); the stored maps are 16-bit tensors, the result and its columns fp32.  Against ``hrnet_ref.backbone`` in float64 the new path and
the fp32-map single-product path (the baseline) are measured on the same case and mode and held to the project's convention
new <= max(1e-4, ``FACTOR`` * baseline); how ``FACTOR`` was fixed from the measured ratios: see ``test_backbone_against_float64``.

Past the 2 GiB window the result's column blocks are fp32 maps of their own and ``torch.cat`` gives the bits of the in-place result.

The switch is inert in every other combination (equal bits, identical launch names), the Res16UNets included.  ``HRNetSeg3S`` and
``HRNetSimCSN3S`` eval logits (separate passes, and the merged-pyramid pass of ``grouped_passes``) with the switch on equal the logits
over the emulated backbone."""
import functools

import pytest
import torch

from tests import hrnet_ref as H
from tests import rows16_ref as R16
from tests import sparse_conv_ref as R
from tests.test_gpu_hrnet import NB_CASES, NETS, SETS, _backbone_inputs, _batch, backbone_reference
from tests.test_gpu_hrnet_infer import N_CONVS, _backbone, _count_calls, _errors, _pyramid, _seg_state

pytestmark = pytest.mark.gpu

M16, S19 = "csn_sparse_conv_bn_act_fwd_m16", "csn_sparse_conv_bn_act_fwd_f32"
CASES = [("s1", 64, 64, 3), ("s1", 256, 256, 3), ("s1", 32, 32, 5), ("s2", 64, 128, 3), ("tr", 128, 64, 3)]
SET_NAMES = ["rand33", "rand129", "rand1031", "two"]
CANARY = -776.0                                      # exact in bf16 and fp16
# new error <= max(1e-4, FACTOR * baseline error) against float64.  The rule was fixed before measuring: a largest measured ratio of at
# most 1.5 keeps the project's factor 2, otherwise the factor is the largest ratio x 1.5 rounded up.  Measured 7.90 (below): 12
FACTOR = 12


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@pytest.fixture(params=["bf16", "fp16"])
def kind(request, L):
    """Math mode 2 / 3 with the single-product instances selected for direct library calls."""
    from csn_amd import functional as CF
    with CF.math_mode(R16.MODES[request.param]), CF.rows16(True):
        yield request.param


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------
# single calls
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(mode, name, c_in, c_out, k):
    """Kernel map (CPU) and float32 CPU tensors of one convolution case, nothing subnormal in fp16; shared, never modified."""
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
    ns = R16.no_subnormals
    return m, ns(t["x"]), ns(t["w"]), vec, ns(r(m.n_out, c_out))


def _block(t, dtype, wide, fill):
    """(n, C) CPU fp32 tensor -> (device view of ``dtype``, its buffer or None); ``wide``: columns [8, 8 + C) of an (n, C + 24) buffer
    of ``fill`` in the same dtype."""
    if not wide:
        return t.cuda().to(dtype).contiguous(), None
    n, C = t.shape
    buf = torch.full((n, C + 24), fill, dtype=dtype, device="cuda")
    buf[:, 8:8 + C] = t.cuda().to(dtype)
    return buf[:, 8:8 + C], buf


def _intact(buf, C, fill):
    return buf is None or (bool((buf[:, :8] == fill).all()) and bool((buf[:, 8 + C:] == fill).all()))


class _Calls:
    """One case on the device: the section-24 call, and the section-19 result for a given (x, r, relu), computed once each."""

    def __init__(self, L, case, kind):
        self.L, self.lib, self.dtype = L, L.lib(), R16.DTYPES[kind]
        m, x_c, w_c, vec, r_c = case
        self.m, self.x_c, self.r_c = m.to("cuda"), x_c, r_c
        self.KV, self.c_in, self.c_out = w_c.shape
        self.w = w_c.cuda().contiguous()
        self.v = {q: t.cuda() for q, t in vec.items()}
        self.refs = {}

    def _vecs(self):
        return [_ptr(self.v[q]) for q in ("gamma", "beta", "mean", "var")]

    def s19(self, x, r, relu):
        """Section 19 on contiguous fp32 tensors."""
        m = self.m
        y = torch.empty(m.n_out, self.c_out, device="cuda")
        self.L.check(self.lib.csn_sparse_conv_bn_act_fwd_f32(
            _ptr(x), x.stride(0), m.n_in, _ptr(m.fwd), m.n_out, self.KV, self.c_in, self.c_out, _ptr(self.w), *self._vecs(), H.EPS, _ptr(r),
            r.stride(0) if r is not None else 0, int(relu), _ptr(y), y.stride(0), _st()), S19)
        return y

    def ref(self, x16, r_key, relu):
        """``y32``: section 19 on fp32 copies of the (already rounded) x and r.  r_key: None, "f32" or "16" (r rounded)."""
        key = (x16, r_key, relu)
        if key not in self.refs:
            rnd = lambda t: t.cuda().to(self.dtype).float()
            x = rnd(self.x_c) if x16 else self.x_c.cuda()
            r = None if r_key is None else (rnd(self.r_c) if r_key == "16" else self.r_c.cuda())
            self.refs[key] = self.s19(x.contiguous(), r, relu)
        return self.refs[key]

    def m16(self, x, r, relu, y):
        m, d = self.m, self.dtype
        self.L.check(self.lib.csn_sparse_conv_bn_act_fwd_m16(
            _ptr(x), int(x.dtype == d), x.stride(0), m.n_in, _ptr(m.fwd), m.n_out, self.KV, self.c_in, self.c_out, _ptr(self.w),
            *self._vecs(), H.EPS, _ptr(r), int(r is not None and r.dtype == d), r.stride(0) if r is not None else 0, int(relu), _ptr(y),
            int(y.dtype == d), y.stride(0), _st()), M16)

    def variant(self, x16, r16, y16, res, relu, wide, twice=False):
        """One call checked against its reference; ``res``: "none", "own" or "alias" (then r16 == y16)."""
        d, C, n_out = self.dtype, self.c_out, self.m.n_out
        ty = lambda flag: d if flag else torch.float32
        x, _ = _block(self.x_c, ty(x16), wide, 1e4)
        r = None
        if res == "own":
            r, _ = _block(self.r_c, ty(r16), wide, 1e4)
        outs = []
        for _rep in range(2 if twice else 1):
            y, ybuf = _block(self.r_c if res == "alias" else torch.full((n_out, C), CANARY), ty(y16), wide, CANARY)
            if res == "alias":
                r = y
            self.m16(x, r, relu, y)
            assert _intact(ybuf, C, CANARY), (x16, r16, y16, res, relu, wide)
            outs.append(y)
        r_key = None if res == "none" else ("16" if (r16 if res == "own" else y16) else "f32")
        y32 = self.ref(x16, r_key, relu)
        want = y32.to(d) if y16 else y32
        assert y.dtype == want.dtype and torch.equal(y, want), (x16, r16, y16, res, relu, wide)
        if twice:
            assert torch.equal(outs[0], outs[1]), "two calls differ"


def _all_variants(L, case, kind):
    c = _Calls(L, case, kind)
    n = 0
    for wide in (False, True):
        for x16 in (0, 1):
            for y16 in (0, 1):
                for res, r16 in (("none", 0), ("own", 0), ("own", 1), ("alias", y16)):
                    for relu in (True, False):
                        c.variant(x16, r16, y16, res, relu, wide, twice=(res == "own" and relu and x16 == y16))
                        n += 1
    # all flags 0: section 24 on fp32 maps IS section 19 (the reference of that variant is the section-19 call on the same tensors)
    assert (0, None, True) in c.refs and (0, "f32", False) in c.refs
    return n


@pytest.mark.parametrize("name", SET_NAMES)
def test_single_calls(L, kind, name):
    n = sum(_all_variants(L, _case(mode, name, c_in, c_out, k), kind) for mode, c_in, c_out, k in CASES)
    print(f"[maps16] single calls {name} {kind}: {n} variants bit-equal to section 19 (rounded once where y is 16-bit)")


def test_single_calls_with_pinned_column_blocks(L, kind):
    lib = L.lib()
    try:
        for c_in, c_out, nb in NB_CASES:
            assert lib.csn_dev_set(L.DEV_SCONV_NB, nb) >= 0
            c = _Calls(L, _case("s1", "rand1031", c_in, c_out, 3), kind)
            for wide in (False, True):
                for relu in (True, False):
                    c.variant(1, 1, 1, "alias", relu, wide)
            c.variant(0, 1, 1, "alias", True, False)                        # the fp32-A instance of the same NB
    finally:
        lib.csn_dev_set(L.DEV_SCONV_NB, 0)


def test_python_call_on_16_bit_tensors(L, kind):
    """``sparse_conv_bn_act`` routes 16-bit tensors and ``out_dtype`` to section 24, takes 16-bit pitched views and accumulates in a
    16-bit buffer; the all-fp32 call without ``out_dtype`` stays section 19."""
    from csn_amd import maps16_dtype, sparse_conv_bn_act, tuning
    from csn_amd.minkowski_hrnet import _pitched16
    d = R16.DTYPES[kind]
    m, x_c, w_c, vec, r_c = _case("s1", "rand129", 64, 64, 3)
    m = m.to("cuda")
    norm = torch.nn.BatchNorm1d(64).cuda().eval()
    with torch.no_grad():
        norm.weight.copy_(vec["gamma"]); norm.bias.copy_(vec["beta"]); norm.running_mean.copy_(vec["mean"]); norm.running_var.copy_(vec["var"])
    w = torch.nn.Parameter(w_c.cuda())
    x16, r16 = x_c.cuda().to(d), r_c.cuda().to(d)
    with tuning.override(rows_single_product=True):
        assert maps16_dtype() is d
        y32, calls = _count_calls(L, lambda: sparse_conv_bn_act(x16.float(), w, m, norm, r16.float(), True))
        assert calls == {S19: 1} and y32.dtype == torch.float32
        got, calls = _count_calls(L, lambda: sparse_conv_bn_act(x16, w, m, norm, r16, True, out_dtype=d))
        assert calls == {M16: 1} and got.dtype == d and got.grad_fn is None and torch.equal(got, y32.to(d))
        # a 16-bit x alone names the route; the result stays fp32 without out_dtype; out_dtype=float32 on fp32 tensors is section 24 too
        got, calls = _count_calls(L, lambda: sparse_conv_bn_act(x16, w, m, norm, r16.float(), True))
        assert calls == {M16: 1} and got.dtype == torch.float32 and torch.equal(got, y32)
        got, calls = _count_calls(L, lambda: sparse_conv_bn_act(x16.float(), w, m, norm, r16.float(), True, out_dtype=torch.float32))
        assert calls == {M16: 1} and torch.equal(got, y32)
        # pitched 16-bit views, in place in a 16-bit buffer
        wide = torch.full((m.n_out, 160), CANARY, device="cuda", dtype=d)
        acc = wide[:, 32:96]
        acc.copy_(r16)
        assert _pitched16(acc) and not acc.is_contiguous()
        assert sparse_conv_bn_act(x16, w, m, norm, acc, True, out=acc) is acc
        assert torch.equal(acc, y32.to(d)) and bool((wide[:, :32] == CANARY).all()) and bool((wide[:, 96:] == CANARY).all())
        # views the kernels cannot take: x / residual are made contiguous, out is refused
        odd = torch.zeros(m.n_out, 68, device="cuda", dtype=d)[:, 4:68]
        odd.copy_(r16)
        assert not _pitched16(odd) and torch.equal(sparse_conv_bn_act(x16, w, m, norm, odd, True, out_dtype=d), y32.to(d))
        with pytest.raises(ValueError, match="out"):
            sparse_conv_bn_act(x16, w, m, norm, None, True, out=odd)


# ------------------------------------------------------------------------------------------------------
# the backbone
# ------------------------------------------------------------------------------------------------------
ON = dict(eval_epilogue=True, rows_single_product=True)


def _emulation(monkeypatch, dtype):
    """``sparse_conv_bn_act`` as the fp32-map launch followed by ONE rounding of the written map, in place — unless the target is a
    column block of the result (a view of the wider buffer)."""
    from csn_amd import minkowski_hrnet as MH
    orig = MH.sparse_conv_bn_act

    def rounded(x, weight, kmap, norm, residual=None, relu=True, out=None, out_dtype=None):
        assert out_dtype is None and x.dtype == torch.float32 and (residual is None or residual.dtype == torch.float32)
        y = orig(x, weight, kmap, norm, residual, relu, out)
        if out is None or out.stride(0) == out.shape[1]:
            y.copy_(y.to(dtype).float())
        return y
    monkeypatch.setattr(MH, "sparse_conv_bn_act", rounded)
    return lambda: monkeypatch.setattr(MH, "sparse_conv_bn_act", orig)


def _result_columns(net):
    S = NETS[net][0]
    return ["bn0s1", f"stages.{S - 1}.0.2.norm2"] + [f"final_transitions.{i - 1}.{3 * (i - 1) + 1}" for i in range(1, S)]


@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_equals_the_rounded_fp32_map_graph(L, kind, net, case, monkeypatch):
    from csn_amd import tuning
    d = R16.DTYPES[kind]
    bb = _backbone(net)
    pyr, feats = _pyramid(net, case)
    t_new, t_emu = {}, {}
    with torch.no_grad(), tuning.override(**ON):
        with tuning.override(infer_maps16=True):
            rows, calls = _count_calls(L, lambda: bb(feats, pyr, t_new))
            again = bb(feats, pyr)
        undo = _emulation(monkeypatch, d)
        emu, c_emu = _count_calls(L, lambda: bb(feats, pyr, t_emu))
        undo()
    # launches: one of section 24 per convolution and nothing of sections 14 / 15 / 19; the emulation is the parent's graph
    assert calls == {M16: N_CONVS[net]}, calls
    assert c_emu == {S19: N_CONVS[net]}, c_emu
    # dtypes and result
    assert rows.dtype == torch.float32 and rows.grad_fn is None and rows.is_contiguous() and torch.equal(rows, again)
    cols = _result_columns(net)
    assert sorted(t_new) == sorted(t_emu) and all(c in t_new for c in cols)
    for k, v in t_new.items():
        assert v.dtype == (torch.float32 if k in cols else d), (k, v.dtype)
    S, ff = NETS[net]
    assert torch.equal(t_new["bn0s1"], rows[:, :32]) and torch.equal(t_new[f"stages.{S - 1}.0.2.norm2"], rows[:, 32:32 + 32 * ff])
    assert torch.equal(t_new[f"final_transitions.{S - 2}.{3 * (S - 2) + 1}"], rows[:, -32 * ff * 2 ** (S - 1):])
    # exactness: the output and every stored map
    assert torch.equal(rows, emu)
    for k in t_new:
        assert torch.equal(t_new[k].float(), t_emu[k]), k
    assert float(rows.abs().max()) > 0 and bool(torch.isfinite(rows).all())


def test_backbone_past_the_window_joins_fp32_maps(L, kind, monkeypatch):
    """Where the result's pitch would pass the 2 GiB window the column blocks are maps of their own, fp32 as in the result:
    ``torch.cat`` converts nothing, and the bits are those of the in-place result."""
    from csn_amd import minkowski_hrnet as MH
    from csn_amd import tuning
    bb = _backbone("2S")
    pyr, feats = _pyramid("2S", "rand300")
    with torch.no_grad(), tuning.override(infer_maps16=True, **ON):
        whole = bb(feats, pyr)
        monkeypatch.setattr(MH, "_WINDOW", 300 * bb.out_channels * 4 - 1)
        trace = {}
        parts, calls = _count_calls(L, lambda: bb(feats, pyr, trace))
    assert calls == {M16: N_CONVS["2S"]} and parts.dtype == torch.float32 and torch.equal(parts, whole)
    cols = _result_columns("2S")
    assert all(v.dtype == (torch.float32 if k in cols else R16.DTYPES[kind]) for k, v in trace.items())


@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_against_float64(L, kind, net, case):
    """Measured on MI355X, error of the 16-bit-map graph / error of the fp32-map single-product graph against float64, y | trace
    (DESIGN.md "16-bit inference maps" has the errors themselves):
        bf16  2S rand300 7.90 | 5.02   2S coarse2 4.28 | 3.73   3S rand300 3.90 | 2.67   3S coarse2 3.11 | 3.11
        fp16  2S rand300 5.75 | 4.36   2S coarse2 4.44 | 4.43   3S rand300 5.62 | 3.36   3S coarse2 2.89 | 2.89
    16-bit residuals and branch sums do NOT stay inside the project's factor 2: a block's residual chain is rounded to 8 (bf16) or
    11 (fp16) bits once per block where the fp32-map graph keeps 24.  Largest ratio 7.90 > 1.5, so ``FACTOR`` = ceil(7.90 x 1.5) = 12."""
    from csn_amd import tuning
    bb = _backbone(net)
    pyr, feats = _pyramid(net, case)
    ref_rows, pre, _ = backbone_reference(net, case, False)
    with torch.no_grad(), tuning.override(**ON):
        t_off, t_on = {}, {}
        rows_off = bb(feats, pyr, t_off)
        with tuning.override(infer_maps16=True):
            rows_on = bb(feats, pyr, t_on)
    base, got = _errors(rows_off, t_off, ref_rows, pre), _errors(rows_on, t_on, ref_rows, pre)
    print(f"[maps16] backbone {net} {case} {kind}: 16-bit maps y {got['y']:.3e} trace {got['trace']:.3e} | fp32 maps y {base['y']:.3e} "
          f"trace {base['trace']:.3e} | ratio y {got['y'] / base['y']:.2f} trace {got['trace'] / base['trace']:.2f}")
    for q in ("y", "trace"):
        assert got[q] <= max(1e-4, FACTOR * base[q]), (q, got[q], base[q])


def _run(L, make, feats, pyr, grad, **switches):
    from csn_amd import tuning
    model = make()
    with torch.set_grad_enabled(grad), tuning.override(**switches):
        rows, calls = _count_calls(L, lambda: model(feats, pyr))
    return rows.detach(), calls, model


@pytest.mark.parametrize("how", ["fp32", "bf16x3", "no_single_product", "grad_enabled", "training", "unfused"])
def test_the_switch_is_inert_elsewhere(L, how):
    from csn_amd import functional as CF
    net = "2S"
    pyr, feats = _pyramid(net, "rand300")
    mode = {"fp32": 0, "bf16x3": 1}.get(how, 2)
    switches = dict(eval_epilogue=True, rows_single_product=how != "no_single_product")
    make = lambda: _backbone(net, fused=how != "unfused", training=how == "training")
    outs = []
    with CF.math_mode(mode):
        for on in (False, True):
            rows, calls, bb = _run(L, make, feats, pyr, how == "grad_enabled", infer_maps16=on, **switches)
            assert M16 not in calls and rows.dtype == torch.float32
            outs.append((rows, calls, bb.bn0s1.running_mean.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    assert (S19 in outs[0][1]) == (how in ("fp32", "bf16x3", "no_single_product"))


def test_the_res16unets_ignore_the_switch(L):
    from csn_amd import functional as CF
    from csn_amd import tuning
    from tests.test_gpu_unet_infer import _model, _pyramid as _unet_pyramid
    pyr, feats = _unet_pyramid(300)
    model = _model("Res16UNet14")
    outs = []
    with CF.math_mode(2), torch.no_grad():
        for on in (False, True):
            with tuning.override(infer_maps16=on, **ON):
                y, calls = _count_calls(L, lambda: model((pyr, feats)))
            assert M16 not in calls and calls.get(S19, 0) > 0
            outs.append((y, calls))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


# ------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------
def test_seg3s_eval_logits_are_the_emulated_backbone_s(L, kind, monkeypatch):
    from csn_amd import HRNetSeg3S, tuning
    model = HRNetSeg3S(3, 6).cuda().eval()
    model.load_state_dict(_seg_state())
    pyr, feats = _pyramid("3S", "rand300")
    with torch.no_grad(), tuning.override(**ON):
        with tuning.override(infer_maps16=True):
            on, calls = _count_calls(L, lambda: model((pyr, feats)))
        undo = _emulation(monkeypatch, R16.DTYPES[kind])
        emu, c_emu = _count_calls(L, lambda: model((pyr, feats)))
        undo()
    # the head and fc_layer see fp32 rows: the same launches either way
    assert calls.get(M16) == 47 and S19 not in calls and c_emu.get(S19) == 47 and M16 not in c_emu and calls.get("csn_rows_fc_fwd_f32") == 1
    assert {k: v for k, v in calls.items() if k != M16} == {k: v for k, v in c_emu.items() if k != S19}
    assert on.dtype == torch.float32 and on.shape == (feats.shape[0], 6) and torch.equal(on, emu)


@pytest.mark.parametrize("grouped", [False, True], ids=["separate", "merged"])
def test_simcsn3s_eval_logits_are_the_emulated_backbone_s(L, kind, grouped, monkeypatch):
    """``grouped``: the merged-pyramid eval pass of ``tuning.grouped_passes`` (one backbone pass over the K + 1 batches)."""
    from csn_amd import HRNetSimCSN3S, tuning
    torch.manual_seed(4)
    model = HRNetSimCSN3S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().eval()
    model.backbone.load_state_dict(H.params(3, 2))
    q, keys = _batch(0), [_batch(1)]
    with torch.no_grad(), tuning.override(grouped_passes=grouped, **ON):
        with tuning.override(infer_maps16=True):
            on, calls = _count_calls(L, lambda: model(q, keys))
        undo = _emulation(monkeypatch, R16.DTYPES[kind])
        emu, c_emu = _count_calls(L, lambda: model(q, keys))
        undo()
    n = 47 if grouped else 2 * 47
    assert calls.get(M16) == n and S19 not in calls and c_emu.get(S19) == n and M16 not in c_emu
    assert {k: v for k, v in calls.items() if k != M16} == {k: v for k, v in c_emu.items() if k != S19}
    assert on.dtype == torch.float32 and torch.equal(on, emu)
