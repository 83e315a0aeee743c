"""fc_layer of the MinkowskiNet head (csn_amd/csrc/rows_fc.hip, include/csn_hip.h section 13), without a GPU: the float64
restatement tests/rows_fc_ref.py against torch's own Linear + BatchNorm1d + ReLU, the host-side argument checks of the raw ABI,
the state dict of a head with and without ``backbone_channels``, and ``load_me_head_state`` on ME-style keys."""
import pytest
import torch
import torch.nn as nn

from tests import rows_fc_ref as R


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_restatement_equals_torch(training):
    n, c_in, c_out, eps, mom = 37, 64, 32, 1e-5, 0.02
    i = R.inputs(3, n, c_in, c_out)
    seq = nn.Sequential(nn.Linear(c_in, c_out), nn.BatchNorm1d(c_out, eps=eps, momentum=mom), nn.ReLU()).double()
    with torch.no_grad():
        seq[0].weight.copy_(i["w"]); seq[0].bias.copy_(i["b"]); seq[1].weight.copy_(i["gamma"]); seq[1].bias.copy_(i["beta"])
        seq[1].running_mean.copy_(i["running_mean"]); seq[1].running_var.copy_(i["running_var"])
    seq.train(training)
    x = i["x"].double().requires_grad_(True)
    y = seq(x)
    (y * i["dy"].double()).sum().backward()
    f = R.fwd(i["x"], i["w"], i["b"], i["gamma"], i["beta"], i["running_mean"], i["running_var"], eps, mom, training)
    b = R.bwd(i["dy"], f["a"] > 0, i["x"], i["w"], i["gamma"], f, training)
    assert (f["y"] - y.detach()).abs().max() < 1e-12
    assert (f["running_mean"] - seq[1].running_mean).abs().max() < 1e-12
    assert (f["running_var"] - seq[1].running_var).abs().max() < 1e-12
    assert int(seq[1].num_batches_tracked) == (1 if training else 0)
    for got, want in ((b["dx"], x.grad), (b["dw"], seq[0].weight.grad), (b["dbias"], seq[0].bias.grad),
                      (b["dgamma"], seq[1].weight.grad), (b["dbeta"], seq[1].bias.grad)):
        assert (got - want).abs().max() < 1e-12


def test_entry_points_reject_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    FAKE = 1 << 20
    ws_f = L.csn_rows_fc_workspace_bytes(13, 64, 32, 1, 0)
    ws_b = L.csn_rows_fc_workspace_bytes(13, 64, 32, 1, 1)
    assert ws_f > 0 and ws_b > 0 and L.csn_rows_fc_workspace_bytes(13, 64, 32, 0, 0) == 0

    def fwd(x=FAKE, ld_x=64, n=13, c_in=64, c_out=32, w=FAKE, training=1, y=FAKE, ld_y=32, z=FAKE, ld_z=32, ws=FAKE, wb=ws_f):
        return L.csn_rows_fc_fwd_f32(x, ld_x, n, c_in, c_out, w, FAKE, FAKE, FAKE, FAKE, FAKE, 1e-5, 0.02, training, y, ld_y, z, ld_z,
                                     FAKE, FAKE, ws, wb, None)
    assert fwd(x=None) == -1 and fwd(w=None) == -1 and fwd(y=None) == -1 and fwd(z=None) == -1 and fwd(ws=None) == -1
    assert fwd(n=0) == -1
    assert fwd(c_in=40, ld_x=40) == -5 and fwd(c_out=48, ld_y=48, ld_z=48) == -5 and fwd(c_in=1056, ld_x=1056) == -5
    assert fwd(ld_x=66) == -2 and fwd(ld_y=34) == -2 and fwd(ld_z=34) == -2
    assert fwd(ld_x=60) == -1                                     # a row shorter than its channels
    assert fwd(x=FAKE + 4) == -3 and fwd(ws=FAKE + 8) == -3
    assert fwd(n=1) == -1                                         # training with one row
    assert fwd(wb=ws_f - 1) == -6

    def bwd(dy=FAKE, ld_dy=32, z=FAKE, ld_x=64, n=13, c_in=64, c_out=32, training=1, dx=FAKE, ld_dx=64, dgamma=FAKE, ws=FAKE, wb=ws_b):
        return L.csn_rows_fc_bwd_f32(dy, ld_dy, FAKE, c_out, z, c_out, FAKE, ld_x, n, c_in, c_out, FAKE, FAKE, FAKE, FAKE, FAKE, 1e-5,
                                     training, dx, ld_dx, FAKE, FAKE, dgamma, FAKE, ws, wb, None)
    assert bwd(dy=None) == -1 and bwd(z=None) == -1 and bwd(dgamma=None) == -1 and bwd(ws=None) == -1
    assert bwd(c_in=40, ld_x=40, ld_dx=40) == -5 and bwd(c_out=48, ld_dy=48) == -5
    assert bwd(ld_dy=34) == -2 and bwd(ld_x=66) == -2 and bwd(ld_dx=66) == -2
    assert bwd(dx=FAKE + 4) == -3
    assert bwd(n=1) == -1
    assert bwd(wb=ws_b - 1) == -6


def test_state_dict_with_and_without_the_backbone_layer():
    from csn_amd.minkowski_csn import BackboneFC, SimCSNHead
    plain = SimCSNHead(64, 2, 5, 1)
    today = ["MHA.w_qs.weight", "MHA.w_ks.weight", "MHA.w_vs.weight", "MHA.fc.weight", "MHA.norm.weight", "MHA.norm.bias",
             "output.weight", "output.bias", "linear_q.weight", "linear_k.weight"]
    assert sorted(plain.state_dict()) == sorted(today)
    assert not hasattr(plain, "fc_layer")
    head = SimCSNHead(64, 2, 5, 1, backbone_channels=416)
    sd = head.state_dict()
    added = {"fc_layer.0.weight": (64, 416), "fc_layer.0.bias": (64,), "fc_layer.1.weight": (64,), "fc_layer.1.bias": (64,),
             "fc_layer.1.running_mean": (64,), "fc_layer.1.running_var": (64,), "fc_layer.1.num_batches_tracked": ()}
    assert sorted(sd) == sorted(today + list(added))
    for name, shape in added.items():
        assert tuple(sd[name].shape) == shape, name
    fc = head.fc_layer
    assert isinstance(fc, BackboneFC) and isinstance(fc[0], nn.Linear) and isinstance(fc[1], nn.BatchNorm1d) and isinstance(fc[2], nn.ReLU)
    assert fc[1].momentum == 0.02 and fc[1].eps == 1e-5
    assert torch.equal(fc[1].weight, torch.ones(64)) and torch.equal(fc[1].bias, torch.zeros(64))
    assert SimCSNHead(64, 2, 5, 1, backbone_channels=480, bn_momentum=0.1).fc_layer[1].momentum == 0.1
    with pytest.raises(ValueError):
        BackboneFC(40, 64)
    with pytest.raises(ValueError):
        BackboneFC(64, 48)


def test_cpu_rows_raise():
    from csn_amd import _lib
    from csn_amd.minkowski_csn import BackboneFC, SimCSNHead
    with pytest.raises(_lib.CsnError):
        BackboneFC(64, 32)(torch.zeros(4, 64))
    with pytest.raises(_lib.CsnError):
        SimCSNHead(32, 2, 5, 0, backbone_channels=64)(torch.zeros(4, 64), [0, 4])


@pytest.mark.parametrize("lead", [False, True], ids=["2d", "me3d"])
def test_load_me_head_state_takes_the_backbone_layer(lead):
    from csn_amd.minkowski_csn import SimCSNHead
    from csn_amd.minkowski_training import load_me_head_state
    g = torch.Generator().manual_seed(5)
    C, c_in, out_ch = 32, 96, 7
    src = SimCSNHead(C, 2, out_ch, 1, backbone_channels=c_in)
    with torch.no_grad():
        for t in src.state_dict().values():
            if t.dtype.is_floating_point:
                t.copy_(torch.randn(t.shape, generator=g))
        src.fc_layer[1].running_var.abs_()
        src.fc_layer[1].num_batches_tracked.fill_(17)
    own = src.state_dict()
    me = {k: v.clone() for k, v in own.items() if k.startswith("MHA.") or k.startswith("linear_")}
    wrap = (lambda t: t[None]) if lead else (lambda t: t)
    me["output.kernel"] = wrap(own["output.weight"].t().clone())
    me["output.bias"] = wrap(own["output.bias"].clone())
    me["fc_layer.0.kernel"] = wrap(own["fc_layer.0.weight"].t().clone())
    me["fc_layer.0.bias"] = wrap(own["fc_layer.0.bias"].clone())
    for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        me[f"fc_layer.1.bn.{leaf}"] = own[f"fc_layer.1.{leaf}"].clone()
    dst = load_me_head_state(SimCSNHead(C, 2, out_ch, 1, backbone_channels=c_in), me)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, own[k]), k
    # a head without the layer ignores the keys, as before
    plain = load_me_head_state(SimCSNHead(C, 2, out_ch, 1), me)
    assert not any(k.startswith("fc_layer") for k in plain.state_dict())
    # wrong shapes and missing keys raise
    for key, bad in (("fc_layer.0.kernel", torch.zeros(C, c_in)), ("fc_layer.0.bias", torch.zeros(C + 1)),
                     ("fc_layer.1.bn.running_var", torch.zeros(C + 1))):
        broken = dict(me)
        broken[key] = bad
        with pytest.raises(ValueError):
            load_me_head_state(SimCSNHead(C, 2, out_ch, 1, backbone_channels=c_in), broken)
    for key in ("fc_layer.0.kernel", "fc_layer.1.bn.num_batches_tracked"):
        broken = {k: v for k, v in me.items() if k != key}
        with pytest.raises(ValueError):
            load_me_head_state(SimCSNHead(C, 2, out_ch, 1, backbone_channels=c_in), broken)
