"""The inference backbone and the plain segmentation networks (csn_amd/minkowski_hrnet.py; include/csn_hip.h section 19), checked
without a GPU: the new export against the header and the ctypes binding; every host-side argument check of
``csn_sparse_conv_bn_act_fwd_f32`` (the codes of section 14, plus the residual's own); ``HRNetSeg2S`` / ``HRNetSeg3S`` state-dict keys
and the checkpoint mapping ``load_me_seg_state``; the refusal of ``HRNetSeg4S``; the ``eval_epilogue`` switch's default."""
import os
import re
import subprocess

import pytest
import torch

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

NAME = "csn_sparse_conv_bn_act_fwd_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------
# the export
# ------------------------------------------------------------------------------------------------------
def test_the_new_export_agrees_with_the_header_and_the_binding():
    from csn_amd import _lib
    _lib.build()
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"CSN_API int " + NAME + r"\(([^;]*)\);", header)
    assert m, "the header does not declare the entry point"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "x", "ld_x", "n_in", "table", "n_out", "kv", "c_in", "c_out", "w", "gamma", "beta", "running_mean", "running_var", "eps", "r",
        "ld_r", "relu", "y", "ld_y", "stream"]
    # the ctypes signature, parameter for parameter
    import ctypes
    kinds = {"*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float}
    want = [kinds["*"] if "*" in p else kinds[" ".join(p.split()[:-1]).replace("const ", "")] for p in params]
    res, args = _lib._SIGNATURES[NAME]
    assert res is ctypes.c_int and args == want
    assert "(19)" in header and header.index("(19)") > header.index("(18)")
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NAME + r"\b", names), "libcsn_hip.so does not export the entry point"
    assert NAME in _lib.EXPORTS and _lib.lib().csn_version() == 17


# ------------------------------------------------------------------------------------------------------
# host-side argument checks of section 19
# ------------------------------------------------------------------------------------------------------
def test_section_19_rejects_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    FAKE, OTHER = 1 << 20, 1 << 22

    # (every call below fails a check: nothing is ever launched on these made-up addresses)
    def f(x=FAKE, ld_x=64, n_in=13, table=FAKE, n_out=11, kv=27, c_in=64, c_out=32, w=FAKE, gamma=FAKE, beta=FAKE, rm=FAKE, rv=FAKE,
          r=OTHER, ld_r=32, relu=1, y=FAKE, ld_y=32):
        return L.csn_sparse_conv_bn_act_fwd_f32(x, ld_x, n_in, table, n_out, kv, c_in, c_out, w, gamma, beta, rm, rv, 1e-5, r, ld_r, relu,
                                                y, ld_y, None)
    ARG, ALIGN, PTR, DIM = -1, -2, -3, -5
    for name in ("x", "table", "w", "gamma", "beta", "rm", "rv", "y"):
        assert f(**{name: None}) == ARG, name
    assert f(n_in=0) == ARG and f(n_out=0) == ARG
    assert f(kv=8) == DIM and f(c_in=40, ld_x=40) == DIM and f(c_out=288, ld_y=288, ld_r=288) == DIM
    assert f(c_in=288, ld_x=288) == DIM and f(c_out=40, ld_y=40, ld_r=40) == DIM and f(c_in=0) == DIM
    # pitches: % 4, at least the width, at most 2^20, and the map inside the 2 GiB window
    assert f(ld_x=66) == ALIGN and f(ld_y=34) == ALIGN and f(ld_r=34) == ALIGN
    assert f(ld_x=60) == ARG and f(ld_y=28) == ARG and f(ld_r=28) == ARG
    assert f(ld_x=(1 << 20) + 4) == DIM and f(ld_y=(1 << 20) + 4) == DIM and f(ld_r=(1 << 20) + 4) == DIM
    assert f(n_in=1 << 24) == DIM and f(n_out=1 << 24) == DIM
    assert f(n_out=1 << 21, ld_y=480, r=None) == DIM and f(n_out=1 << 21, ld_y=32, ld_r=480) == DIM
    # alignment
    assert f(x=FAKE + 4) == PTR and f(w=FAKE + 8) == PTR and f(y=FAKE + 4) == PTR and f(r=OTHER + 8) == PTR and f(table=FAKE + 2) == PTR
    # the residual: ignored when NULL (its pitch with it); y itself only element for element
    assert f(r=None, ld_r=0, ld_y=28) == ARG and f(r=None, ld_r=3, x=FAKE + 4) == PTR
    assert f(r=FAKE, ld_r=64, ld_y=32) == ARG and f(r=FAKE, ld_r=32, ld_y=64) == ARG
    assert f(r=FAKE, ld_r=64, ld_y=64, x=FAKE + 4) == PTR                   # r == y at one pitch passes the aliasing rule


def test_the_window_check_is_reached_with_a_valid_call_shape():
    """The last of the checks before the launch: a call whose every other argument is valid and whose ``y`` pitch alone takes the map
    past 2 GiB (what ``HRNetBackbone`` tests before it writes the concatenated result in place)."""
    from csn_amd import _lib
    from csn_amd.minkowski_hrnet import _WINDOW
    _lib.build()
    L = _lib.lib()
    FAKE = 1 << 20
    n = _WINDOW // (480 * 4) + 1
    call = lambda rows: L.csn_sparse_conv_bn_act_fwd_f32(FAKE, 32, rows, FAKE, rows, 27, 32, 32, FAKE, FAKE, FAKE, FAKE, FAKE, 1e-5, None,
                                                         0, 1, FAKE, 480, None)
    assert n * 480 * 4 > _WINDOW >= (n - 1) * 480 * 4 and call(n) == -5


# ------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------
SEG = {"2S": (2, 224), "3S": (3, 480)}


@pytest.mark.parametrize("net", ["2S", "3S"])
def test_seg_state_dict_keys(net):
    import csn_amd
    from csn_amd.minkowski_csn import BackboneFC
    S, width = SEG[net]
    model = getattr(csn_amd, f"HRNetSeg{net}")(3, 7)
    assert model.FEAT_FACTOR == 2 and model.NUM_STAGES == S and model.backbone.out_channels == width
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {f"backbone.{k}": v for k, v in H.param_shapes(S, 2).items()}
    want.update({"final.0.weight": (256, width), "final.0.bias": (256,), "final.1.weight": (256,), "final.1.bias": (256,),
                 "final.1.running_mean": (256,), "final.1.running_var": (256,), "final.1.num_batches_tracked": (),
                 "final.3.weight": (7, 256), "final.3.bias": (7,)})
    assert got == want
    assert isinstance(model.final, BackboneFC) and isinstance(model.final[3], torch.nn.Linear) and len(model.final) == 4
    assert model.final[1].momentum == 0.02 and float(model.final[1].weight.detach().min()) == 1.0


def _reference_named(sd):
    """Our state dict under the reference's names: backbone modules at the top level, norms behind ``.bn``, ``final.0`` / ``final.3``
    as MinkowskiEngine kernels (1, c_in, c_out) with (1, c_out) biases."""
    out = {}
    for k, v in sd.items():
        if k.startswith("backbone."):
            k = k[len("backbone."):]
            mod, leaf = k.rsplit(".", 1)
            out[k if leaf == "kernel" else f"{mod}.bn.{leaf}"] = v.clone()
        elif k in ("final.0.weight", "final.3.weight"):
            out[k.replace("weight", "kernel")] = v.t().clone().unsqueeze(0)
        elif k in ("final.0.bias", "final.3.bias"):
            out[k] = v.clone().unsqueeze(0)
        else:
            out["final.1.bn." + k[len("final.1."):]] = v.clone()
    return out


@pytest.mark.parametrize("net", ["2S", "3S"])
def test_load_me_seg_state_round_trips_and_refuses_bad_checkpoints(net):
    import csn_amd
    from csn_amd import load_me_seg_state
    cls = getattr(csn_amd, f"HRNetSeg{net}")
    torch.manual_seed(1)
    src, dst = cls(3, 7), cls(3, 7)
    with torch.no_grad():
        for v in src.state_dict().values():
            if v.is_floating_point():
                v.normal_()
            else:
                v.fill_(5)
    ref_sd = _reference_named(src.state_dict())
    assert {"conv0s1.kernel", "final.0.kernel", "final.0.bias", "final.1.bn.running_var", "final.3.kernel", "final.3.bias"} <= set(ref_sd)
    assert not any(k.startswith("final.2") for k in ref_sd)
    assert load_me_seg_state(dst, ref_sd) is dst
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # MinkowskiEngine's other documented layout: (c_in, c_out) kernels and flat biases
    flat = {k: (v[0] if k in ("final.0.kernel", "final.0.bias", "final.3.kernel", "final.3.bias") else v) for k, v in ref_sd.items()}
    again = load_me_seg_state(cls(3, 7), flat).state_dict()
    assert all(torch.equal(a[k], again[k]) for k in a)
    for missing in ("final.0.kernel", "final.0.bias", "final.1.bn.running_mean", "final.3.kernel", "final.3.bias", "bn0s1.bn.weight"):
        bad = {k: v for k, v in ref_sd.items() if k != missing}
        with pytest.raises(ValueError, match=re.escape(missing)):
            load_me_seg_state(dst, bad)
    for name, shape in (("final.3.kernel", (1, 256, 8)), ("final.0.kernel", (1, 256, 256)), ("final.3.bias", (1, 8)),
                        ("final.1.bn.weight", (128,)), ("stages.0.0.1.conv2.kernel", (27, 128, 64))):
        bad = dict(ref_sd)
        bad[name] = torch.zeros(shape)
        with pytest.raises(ValueError, match=re.escape(name)):
            load_me_seg_state(dst, bad)
    # a refused checkpoint leaves the model as it was
    b = dst.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_simcsn_checkpoints_load_as_before():
    """``load_me_hrnet_state`` shares its backbone half with ``load_me_seg_state``: a seg checkpoint is no SimCSN checkpoint."""
    from csn_amd import HRNetSeg2S
    from csn_amd.minkowski_hrnet import HRNetSimCSN2S, load_me_hrnet_state
    ref_sd = _reference_named(HRNetSeg2S(3, 7).state_dict())
    with pytest.raises(ValueError):
        load_me_hrnet_state(HRNetSimCSN2S(3, 7, d_model=64, n_head=2), ref_sd)


def test_seg_4s_is_refused_and_cpu_tensors_raise():
    from csn_amd import CsnError, HRNetSeg2S, HRNetSeg4S, build_pyramid, sparse_conv_bn_act, tuning
    with pytest.raises(NotImplementedError, match="512"):
        HRNetSeg4S(3, 5)
    pts = torch.tensor(R.dense_block())
    pyr = build_pyramid(pts, 2)
    model = HRNetSeg2S(3, 5).eval()
    with pytest.raises(CsnError):
        model((pts, torch.zeros(64, 3)))
    with torch.no_grad(), tuning.override(eval_epilogue=True), pytest.raises(CsnError):
        model((pyr, torch.zeros(64, 3)))
    with pytest.raises(CsnError):
        sparse_conv_bn_act(torch.zeros(64, 32), torch.zeros(27, 32, 32), pyr.s1[0], torch.nn.BatchNorm1d(32))


def test_the_switch_defaults_to_off():
    from csn_amd import tuning
    assert tuning.Tuning().eval_epilogue is False and tuning.current().eval_epilogue is False
    with tuning.override(eval_epilogue=True) as t:
        assert t.eval_epilogue and tuning.current().eval_epilogue
    assert tuning.current().eval_epilogue is False
