"""The HRNet backbone on voxel rows (csn_amd/minkowski_hrnet.py; include/csn_hip.h section 15), checked without a GPU:
the float64 restatement tests/hrnet_ref.py against the same 2S / 3S networks written with torch's dense conv3d / conv_transpose3d
/ batch_norm on a fully occupied 8^3 block of two shapes (the only independent pin of the exchange wiring; bound 1e-10);
``build_pyramid`` against ``down_coords`` / ``geometry`` (negative coordinates included); the backbone's parameter names and shapes
against a list written out from hrnet.py's constructor; ``load_me_hrnet_state``; the host-side argument checks of section 15; and
the decidedness of every ReLU mask the GPU tests compare (asserted on the reference alone)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

NETS = {"2S": (2, 4), "3S": (3, 2)}


# ------------------------------------------------------------------------------------------------------
# the restatement against dense torch
# ------------------------------------------------------------------------------------------------------
def _dense_weight(w, k, transposed=False):
    v = w.reshape(k, k, k, w.shape[1], w.shape[2])                       # [oz][oy][ox][ci][co]
    return v.permute(3, 4, 0, 1, 2) if transposed else v.permute(4, 3, 0, 1, 2)


def _dense_backbone(vol, p, num_stages, training):
    """hrnet.py:122-163 + 308-326 + 433-437 on dense (B, C, Z, Y, X) volumes: every level is fully occupied, so the sparse
    convolutions are torch's dense ones with zero padding."""
    def bn(z, name):
        return F.batch_norm(z, p[name + ".running_mean"].clone(), p[name + ".running_var"].clone(), p[name + ".weight"],
                            p[name + ".bias"], training, H.MOMENTUM, H.EPS)
    c1 = lambda x, n, k=3: F.conv3d(x, _dense_weight(p[n + ".kernel"], k), padding=k // 2)
    dn = lambda x, n: F.conv3d(x, _dense_weight(p[n + ".kernel"], 3), stride=2, padding=1)
    up = lambda x, n: F.conv_transpose3d(x, _dense_weight(p[n + ".kernel"], 3, True), stride=2, padding=1, output_padding=1)
    out_init = F.relu(bn(c1(vol, "conv0s1", 5), "bn0s1"))
    out = F.relu(bn(c1(out_init, "conv1s1"), "bn1s1"))
    stage_input = [out]
    for i in range(num_stages):
        stage_output = []
        for j in range(i + 1):
            x = stage_input[j]
            for b in range(3):
                n = f"stages.{i}.{j}.{b}."
                h = F.relu(bn(c1(x, n + "conv1"), n + "norm1"))
                x = F.relu(bn(c1(h, n + "conv2"), n + "norm2") + x)
            stage_output.append(x)
        if i == num_stages - 1:
            break
        depth = len(stage_output)
        nxt = [[] for _ in range(depth + 1)]
        for j in range(depth):
            for k in range(depth + 1):
                if j == k:
                    nxt[k].append(stage_output[j])
                    continue
                # nn.Sequential of hrnet.py:82-118: conv, norm, (relu, conv, norm)*
                t = stage_output[j]
                for s in range(abs(k - j)):
                    if s:
                        t = F.relu(t)
                    n = f"exchange_blocks.{i}.{j}.{k}."
                    t = bn((dn if k > j else up)(t, n + str(3 * s)), n + str(3 * s + 1))
                nxt[k].append(t)
        stage_input = []
        for parts in nxt:
            buf = parts[0]
            for t in parts[1:]:
                buf = buf + t
            stage_input.append(F.relu(buf))
    outs = [out_init, stage_output[0]]
    for i in range(1, num_stages):
        x = stage_output[i]
        for s in range(i):
            n = f"final_transitions.{i - 1}."
            x = F.relu(bn(up(x, n + str(3 * s)), n + str(3 * s + 1)))
        outs.append(x)
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("net", ["2S", "3S"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_restatement_equals_dense_torch(net, training):
    S, ff = NETS[net]
    side = 8
    coords = [(b, x, y, z) for b in range(2) for z in range(side) for y in range(side) for x in range(side)]    # rows (b, z, y, x)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in H.params(S, ff).items()}
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(len(coords), 3, generator=g).double()
    rows, _, _ = H.backbone(H.Pyramid(coords, S), feats, p, S, training)
    vol = feats.reshape(2, side, side, side, 3).permute(0, 4, 1, 2, 3)
    dense = _dense_backbone(vol, p, S, training).permute(0, 2, 3, 4, 1).reshape(len(coords), -1)
    err = (rows - dense).abs().max().item()
    print(f"[hrnet] {net} {'train' if training else 'eval'}: restatement vs dense torch {err:.2e}")
    assert rows.shape[1] == {"2S": 416, "3S": 480}[net]
    assert err < 1e-10


# ------------------------------------------------------------------------------------------------------
# the pyramid
# ------------------------------------------------------------------------------------------------------
def _tables_from(g):
    t = torch.full((g.KV, g.n_out), -1, dtype=torch.int32)
    for k, (j, i) in enumerate(g.pairs):
        t[k, j] = i.int()
    return t


def test_pyramid_levels_and_maps_agree_with_the_dictionary():
    from csn_amd.minkowski_hrnet import build_pyramid
    pts = R.random_set(300)
    assert min(min(c[1:]) for c in pts) < 0                                # negative coordinates included
    pyr = build_pyramid(torch.tensor(pts), 3, stem_kernel=5)
    ref = H.Pyramid(pts, 3)
    assert pyr.n_levels == 3 and pyr.stem.kernel_size == 5 and pyr.stem.KV == 125
    lvl = [tuple(c) for c in pts]
    for l in range(3):
        assert [tuple(c) for c in pyr.coords[l].tolist()] == ref.coords[l]
        if l:
            lvl = R.down_coords(lvl, 1 << (l - 1))
            assert ref.coords[l] == lvl
        assert torch.equal(pyr.s1[l].fwd, _tables_from(ref.s1[l])) and pyr.s1[l].in_tensor_stride == 1 << l
    assert torch.equal(pyr.stem.fwd, _tables_from(ref.stem))
    for l in range(2):
        assert torch.equal(pyr.down[l].fwd, _tables_from(ref.down[l]))
        up = pyr.up(l)
        assert up.transposed and torch.equal(up.fwd, _tables_from(ref.up[l])) and up.n_out == len(ref.coords[l])
    moved = pyr.to("cpu")
    assert torch.equal(moved.down[1].fwd, pyr.down[1].fwd) and moved.n_levels == 3
    tiny = build_pyramid(torch.tensor(H.two_coarse_rows(3)), 3)
    assert tiny.coords[2].shape[0] == 2
    assert build_pyramid(torch.tensor(H.two_coarse_rows(2)), 2).coords[1].shape[0] == 2


# ------------------------------------------------------------------------------------------------------
# names, shapes, checkpoints
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["2S", "3S"])
def test_backbone_names_and_shapes(net):
    from csn_amd.minkowski_hrnet import HRNetBackbone
    S, ff = NETS[net]
    bb = HRNetBackbone(3, S, ff)
    want = H.param_shapes(S, ff)
    got = {k: tuple(v.shape) for k, v in bb.state_dict().items()}
    assert got == want
    assert bb.out_channels == {"2S": 416, "3S": 480}[net]
    n_pairs = sum(1 for k in want if k.endswith(".kernel"))
    assert n_pairs == {"2S": 2 + 18 + 1 + 1, "3S": 47}[net]              # convolution + BatchNorm pairs of one pass
    # a few names spelled out from hrnet.py:82-118: a two-step path is conv 0, norm 1, relu 2, conv 3, norm 4
    if net == "3S":
        assert want["exchange_blocks.1.0.2.3.kernel"] == (27, 128, 256) and want["exchange_blocks.1.0.2.4.weight"] == (256,)
        assert want["exchange_blocks.1.1.0.0.kernel"] == (27, 128, 64) and want["final_transitions.1.3.kernel"] == (27, 256, 256)
        assert "exchange_blocks.1.0.2.2.kernel" not in want
    assert all(float(m.weight.detach().min()) == 1.0 and float(m.bias.detach().abs().max()) == 0.0 for m in bb.modules()
               if isinstance(m, torch.nn.BatchNorm1d))
    assert bb.bn0s1.momentum == 0.02


def test_block_keys_are_those_of_sparse_basic_block():
    from csn_amd import SparseBasicBlock
    from csn_amd.minkowski_hrnet import HRBasicBlock
    assert list(HRBasicBlock(64, 64).state_dict()) == list(SparseBasicBlock(64, 64).state_dict())


def test_4s_is_refused_and_cpu_rows_raise():
    from csn_amd import CsnError
    from csn_amd.minkowski_hrnet import HRNetBackbone, HRNetSimCSN4S, bn_act, build_pyramid, conv_stats
    with pytest.raises(NotImplementedError, match="512"):
        HRNetSimCSN4S(3, 5)
    with pytest.raises(NotImplementedError):
        HRNetBackbone(3, 4, 2)
    pts = torch.tensor(R.dense_block())
    pyr = build_pyramid(pts, 2)
    for fused in (True, False):
        with pytest.raises(CsnError):
            HRNetBackbone(3, 2, 4, fused=fused)(torch.zeros(64, 3), pyr)
    with pytest.raises(CsnError):
        conv_stats(torch.zeros(64, 32), torch.zeros(27, 32, 32), pyr.s1[0], None, None, 1e-5, 0.02)
    v = torch.zeros(32)
    with pytest.raises(CsnError):
        bn_act([(torch.zeros(4, 32), v, v, v, v)])


def _reference_named(model_sd):
    """Our state dict under the reference's names: backbone modules at the top level, norms behind ``.bn``, the head's fc_layer /
    output as MinkowskiEngine kernels."""
    out = {}
    for k, v in model_sd.items():
        if k.startswith("backbone."):
            k = k[len("backbone."):]
            mod, leaf = k.rsplit(".", 1)
            out[k if leaf == "kernel" else f"{mod}.bn.{leaf}"] = v.clone()
        elif k.startswith("head."):
            k = k[len("head."):]
            if k == "output.weight":
                out["output.kernel"] = v.t().clone().unsqueeze(0)
            elif k == "fc_layer.0.weight":
                out["fc_layer.0.kernel"] = v.t().clone().unsqueeze(0)
            elif k.startswith("fc_layer.1."):
                out["fc_layer.1.bn." + k[len("fc_layer.1."):]] = v.clone()
            elif k in ("output.bias", "fc_layer.0.bias"):
                out[k] = v.clone().unsqueeze(0)
            else:
                out[k] = v.clone()
    return out


def test_load_me_hrnet_state_round_trips_and_refuses_a_wrong_shape():
    from csn_amd.minkowski_hrnet import HRNetSimCSN2S, load_me_hrnet_state
    torch.manual_seed(0)
    src, dst = HRNetSimCSN2S(3, 7, d_model=64, n_head=2), HRNetSimCSN2S(3, 7, d_model=64, n_head=2)
    with torch.no_grad():
        for v in src.state_dict().values():
            if v.is_floating_point():
                v.normal_()
            else:
                v.fill_(5)
    ref_sd = _reference_named(src.state_dict())
    assert "conv0s1.kernel" in ref_sd and "exchange_blocks.0.0.1.1.bn.running_var" in ref_sd and "stages.1.1.2.norm2.bn.weight" in ref_sd
    load_me_hrnet_state(dst, ref_sd)
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    bad = dict(ref_sd)
    bad["stages.0.0.1.conv2.kernel"] = torch.zeros(27, 128, 64)
    with pytest.raises(ValueError, match="stages.0.0.1.conv2.kernel"):
        load_me_hrnet_state(dst, bad)
    del bad["stages.0.0.1.conv2.kernel"]
    with pytest.raises(ValueError):
        load_me_hrnet_state(dst, bad)


# ------------------------------------------------------------------------------------------------------
# host-side argument checks of section 15
# ------------------------------------------------------------------------------------------------------
def test_section_15_rejects_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    FAKE = 1 << 20
    ws_a = L.csn_sparse_conv_stats_workspace_bytes(11, 32)
    assert ws_a > 0 and L.csn_sparse_conv_stats_workspace_bytes(0, 32) == 0 and L.csn_sparse_conv_stats_workspace_bytes(11, 48) == 0

    def cs(x=FAKE, ld_x=64, n_in=13, table=FAKE, n_out=11, kv=27, c_in=64, c_out=32, w=FAKE, z=FAKE, ld_z=32, mean=FAKE, invstd=FAKE,
           rm=None, rv=None, ws=FAKE, wb=ws_a):
        return L.csn_sparse_conv_stats_fwd_f32(x, ld_x, n_in, table, n_out, kv, c_in, c_out, w, z, ld_z, mean, invstd, rm, rv, 1e-5, 0.02,
                                               ws, wb, None)
    for name in ("x", "table", "w", "z", "mean", "invstd", "ws"):
        assert cs(**{name: None}) == -1, name
    assert cs(n_out=1) == -1                                               # a single voxel has no variance
    assert cs(n_in=0) == -1 and cs(kv=8) == -5 and cs(c_in=40, ld_x=40) == -5 and cs(c_out=288, ld_z=288) == -5
    assert cs(ld_x=66) == -2 and cs(ld_z=34) == -2 and cs(ld_z=28) == -1
    assert cs(x=FAKE + 4) == -3 and cs(z=FAKE + 8) == -3 and cs(ws=FAKE + 4) == -3 and cs(table=FAKE + 2) == -3
    assert cs(wb=ws_a - 1) == -6

    ws_b = L.csn_rows_bn_act_workspace_bytes(65, 64, 2)
    assert ws_b > 0 and L.csn_rows_bn_act_workspace_bytes(65, 64, 4) == 0 and L.csn_rows_bn_act_workspace_bytes(65, 40, 1) == 0

    def terms(M=2, ld=64, **over):
        t = _lib.BnTerms()
        for m in range(M):
            t.z[m], t.ld_z[m], t.mean[m], t.scale[m], t.gamma[m], t.beta[m] = FAKE, ld, FAKE, FAKE, FAKE, FAKE
            t.dz[m], t.ld_dz[m], t.dgamma[m], t.dbeta[m] = FAKE, ld, FAKE, FAKE
        for k, (m, v) in over.items():
            getattr(t, k)[m] = v
        return t

    def fw(t=None, M=2, n=65, C=64, r=FAKE, ld_r=64, y=FAKE, ld_y=64):
        t = terms(M if 1 <= M <= 3 else 1) if t is None else t
        return L.csn_rows_bn_act_fwd_f32(ctypes.addressof(t), M, n, C, 1, 1e-5, r, ld_r, 1, y, ld_y, None)
    assert L.csn_rows_bn_act_fwd_f32(None, 1, 65, 64, 1, 1e-5, None, 0, 1, FAKE, 64, None) == -1
    assert fw(M=0) == -1 and fw(M=4) == -1 and fw(n=0) == -1 and fw(y=None) == -1
    assert fw(C=40) == -5 and fw(C=288) == -5
    assert fw(t=terms(z=(1, None))) == -1 and fw(t=terms(beta=(0, None))) == -1 and fw(t=terms(scale=(1, None))) == -1
    assert fw(t=terms(ld_z=(1, 66))) == -2 and fw(t=terms(ld_z=(0, 60))) == -1 and fw(t=terms(z=(1, FAKE + 4))) == -3
    assert fw(ld_y=66) == -2 and fw(ld_y=60) == -1 and fw(ld_r=62) == -1 and fw(y=FAKE + 4) == -3 and fw(r=FAKE + 8) == -3
    assert fw(n=1 << 24) == -5

    def bw(t=None, M=2, n=65, C=64, dy=FAKE, ld_dy=64, y=FAKE, ld_y=64, relu=1, dr=FAKE, ld_dr=64, ws=FAKE, wb=ws_b):
        t = terms(M if 1 <= M <= 3 else 1) if t is None else t
        return L.csn_rows_bn_act_bwd_f32(dy, ld_dy, y, ld_y, ctypes.addressof(t), M, n, C, 1, 1e-5, relu, dr, ld_dr, ws, wb, None)
    assert bw(dy=None) == -1 and bw(ws=None) == -1 and bw(y=None) == -1 and bw(M=0) == -1 and bw(M=4) == -1
    assert bw(C=48) == -5 and bw(ld_dy=66) == -2 and bw(ld_dr=60) == -1 and bw(ld_y=34) == -1
    assert bw(t=terms(gamma=(1, None))) == -1 and bw(t=terms(ld_dz=(0, 66))) == -2 and bw(t=terms(dz=(1, FAKE + 4))) == -3
    assert bw(dy=FAKE + 4) == -3 and bw(dr=FAKE + 8) == -3 and bw(ws=FAKE + 8) == -3
    assert bw(wb=ws_b - 1) == -6


# ------------------------------------------------------------------------------------------------------
# mask decidedness of the GPU tests' cases
# ------------------------------------------------------------------------------------------------------
def _undecided(a):
    return (a.abs() < 1e-4).double().mean().item()


@pytest.mark.parametrize("net", ["2S", "3S"])
@pytest.mark.parametrize("case", ["rand300", "coarse2"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_backbone_cases_have_decided_relu_masks(net, case, training):
    """tests/test_gpu_hrnet.py takes gradients under the GPU's own masks and compares outputs with true ReLUs; both rest on the
    float64 pre-activations being away from zero: at most 0.1 % of each may lie within 1e-4 of it."""
    _, pre = backbone_case(net, case, training)[:2]
    # (sum.0.0 is the ReLU of a block's output alone — no path comes in after stage 0 — so its zeros are exact, not undecided)
    worst = max(_undecided(a) for k, a in pre.items() if k != "sum.0.0")
    print(f"[hrnet] {net} {case} {'train' if training else 'eval'}: undecided share, worst ReLU {worst:.2e}")
    assert worst <= 1e-3


def backbone_case(net, case, training):
    from tests.test_gpu_hrnet import backbone_reference
    return backbone_reference(net, case, training)


def test_bn_act_cases_have_decided_relu_masks():
    from tests.test_gpu_hrnet import bn_act_case
    for M in (1, 2, 3):
        for n in (2, 63, 65, 1031):
            for C in (32, 96, 256):
                for training in (True, False):
                    c = bn_act_case(M, n, C)
                    terms = [dict(z=t["z"].double(), gamma=t["gamma"].double(), beta=t["beta"].double(),
                                  running_mean=t["running_mean"].double(), running_var=t["running_var"].double()) for t in c["terms"]]
                    for r in (None, c["r"].double()):
                        _, a = H.bn_act(terms, r, True, training)
                        assert _undecided(a) <= 1e-3, (M, n, C, training)
