"""Host-side checks (no GPU) of the kernel-2 stride-2 convolutions and the Res16UNet family: ``build_octant_map`` against the
dictionary restatement tests/octant_ref.py on every point set the GPU tests use, at tensor strides 1 and 2, with negative
coordinates and shuffled rows; what the map refuses; the argument checks of include/csn_hip.h section 21 (made before any launch);
the ABI's header <-> exports equality; the classes' refusals, state-dict key sets and ``load_me_unet_state``; the ``train_seg``
parser."""
import random

import pytest
import torch

from tests import octant_ref as O
from tests import sparse_conv_ref as R
from tests import unet_ref as U

SETS = {"single": R.single_voxel, "dense4": R.dense_block, "rand33": lambda ts=1: R.random_set(33, ts=ts),
        "rand129": lambda ts=1: R.random_set(129, ts=ts), "rand300": lambda ts=1: R.random_set(300, ts=ts),
        "rand1031": lambda ts=1: R.random_set(1031, ts=ts), "clusters": R.two_clusters, "even_y": lambda ts=1: O.even_y(ts=ts)}


def _check_map(pts, ts):
    from csn_amd.minkowski_conv import build_kernel_map, build_octant_map
    p = O.Partition(pts, ts)
    m = build_octant_map(torch.tensor(pts), tensor_stride=ts)
    assert (m.in_tensor_stride, m.out_tensor_stride, m.n_fine, m.n_coarse) == (ts, 2 * ts, p.n_fine, p.n_coarse)
    for t in (m.parent, m.octant, m.children, m.order, m.seg):
        assert t.dtype == torch.int32
    assert m.in_coords.tolist() == [list(c) for c in pts] and m.out_coords.tolist() == [list(c) for c in p.coarse]
    assert m.parent.tolist() == p.parent and m.octant.tolist() == p.octant and m.children.tolist() == p.children
    assert tuple(m.children.shape) == (8, p.n_coarse) and tuple(m.seg.shape) == (9,)
    # order / seg: the stable sort by octant
    want = sorted(range(p.n_fine), key=lambda i: (p.octant[i], i))
    assert m.order.tolist() == want
    seg = m.seg.tolist()
    assert seg[0] == 0 and seg[8] == p.n_fine and [b - a for a, b in zip(seg, seg[1:])] == p.segments()
    for k in range(8):
        assert all(p.octant[i] == k for i in want[seg[k]:seg[k + 1]])
    # children and (parent, octant) are inverse to each other
    rows = torch.arange(p.n_fine, dtype=torch.int32)
    assert torch.equal(m.children[m.octant.long(), m.parent.long()], rows)
    hit = m.children >= 0
    assert int(hit.sum()) == p.n_fine
    k_of, j_of = torch.nonzero(hit, as_tuple=True)
    assert torch.equal(m.octant[m.children[hit].long()].long(), k_of) and torch.equal(m.parent[m.children[hit].long()].long(), j_of)
    # the coarse set is the one the kernel-3 stride-2 map generates
    assert torch.equal(m.out_coords, build_kernel_map(torch.tensor(pts), kernel_size=3, stride=2, tensor_stride=ts).out_coords)
    return p, m


@pytest.mark.parametrize("ts", [1, 2])
@pytest.mark.parametrize("name", list(SETS))
def test_octant_map_against_the_dictionary_restatement(name, ts):
    pts = SETS[name](ts=ts)
    assert name in ("dense4", "clusters") or min(min(c[1:]) for c in pts) < 0                # negative coordinates are covered
    _check_map(pts, ts)
    shuffled = list(pts)
    random.Random(len(pts)).shuffle(shuffled)
    _check_map(shuffled, ts)


def test_derived_levels_and_segment_sizes():
    """The segment sizes the GPU tests rely on, and the five levels of the network tests' sets."""
    seg = lambda pts, ts=1: sorted(O.Partition(pts, ts).segments())
    assert seg(R.random_set(33))[0] >= 1 and seg(R.random_set(33))[-1] <= 8
    assert seg(R.random_set(129))[0] >= 7 and seg(R.random_set(129))[-1] <= 23
    s = seg(R.random_set(1031))
    assert s[0] >= 115 and s[-1] <= 142 and s[0] < 128 < s[-1]
    assert seg(R.two_clusters())[-1] == 180 and 9 <= seg(R.two_clusters())[0] and seg(R.two_clusters())[-2] <= 27
    l3, ts3 = O.level(R.two_clusters(), 1, 3)
    assert ts3 == 8 and seg(l3, ts3).count(0) == 4
    _check_map(l3, ts3)
    assert seg(R.dense_block()) == [8] * 8
    for n in (300, 1031):
        sizes = [len(O.level(R.random_set(n), 1, l)[0]) for l in range(5)]
        assert sizes[0] == n and min(sizes) >= 16, sizes                                     # no BatchNorm sees fewer than 16 rows


def test_octant_map_floors_negative_coordinates_and_takes_given_out_coords():
    from csn_amd.minkowski_conv import build_octant_map
    coords = torch.tensor([[0, -1, -2, -3], [0, 1, 0, -4], [0, -5, 3, 2]])
    m = build_octant_map(coords)
    assert m.out_coords.tolist() == [[0, -6, 2, 2], [0, -2, -2, -4], [0, 0, 0, -4]]           # floor: -1 -> -2, -3 -> -4, -5 -> -6
    assert m.parent.tolist() == [1, 2, 0] and m.octant.tolist() == [1 + 0 + 4, 1, 1 + 2]
    given = torch.tensor([[0, 0, 0, -4], [1, 0, 0, 0], [0, -2, -2, -4], [0, -6, 2, 2]])       # a superset, in another order
    g = build_octant_map(coords, out_coords=given)
    assert g.parent.tolist() == [2, 0, 3] and g.octant.tolist() == m.octant.tolist() and tuple(g.children.shape) == (8, 4)
    assert g.children[5, 2] == 0 and int((g.children >= 0).sum()) == 3
    with pytest.raises(ValueError, match="misses the parent"):
        build_octant_map(coords, out_coords=given[:3])


def test_octant_map_refuses_what_it_does_not_take():
    from csn_amd.minkowski_conv import build_octant_map
    bad = [dict(coords=torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3]])),                           # duplicate rows
           dict(coords=torch.tensor([[0, 1, 0, 0]]), tensor_stride=2),                        # not a multiple of the tensor stride
           dict(coords=torch.tensor([[0, 0, 0, 0]]), tensor_stride=0),
           dict(coords=torch.tensor([[1 << 15, 0, 0, 0]])), dict(coords=torch.tensor([[0, 1 << 15, 0, 0]])),
           dict(coords=torch.tensor([[0, 0, 0, 0]]), out_coords=torch.tensor([[0, 1, 0, 0]])),   # out_coords off its stride
           dict(coords=torch.tensor([[0, 0, 0, 0]]), out_coords=torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0]])),
           dict(coords=torch.zeros(0, 4, dtype=torch.long)), dict(coords=torch.zeros(3, 3, dtype=torch.long))]
    for kw in bad:
        with pytest.raises(ValueError):
            build_octant_map(**kw)


# ------------------------------------------------------------------------------------------------------
# raw ABI, host side
# ------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    F = 1 << 20
    ws = {up: L.csn_octant_conv_workspace_bytes(13, 11, 64, 32, up, 1) for up in (0, 1)}
    assert ws[0] > 0 and ws[1] > 0 and L.csn_octant_conv_workspace_bytes(13, 11, 64, 32, 0, 0) == 0
    assert L.csn_octant_conv_workspace_bytes(13, 11, 40, 32, 0, 1) == 0 and L.csn_octant_conv_workspace_bytes(0, 11, 64, 32, 1, 1) == 0

    def down(x=F, ld_x=64, n_fine=13, ch=F, n_coarse=11, c_in=64, c_out=32, w=F, bias=None, y=F, ld_y=32):
        return L.csn_octant_down_fwd_f32(x, ld_x, n_fine, ch, n_coarse, c_in, c_out, w, bias, y, ld_y, None)

    def up(x=F, ld_x=64, n_coarse=11, par=F, order=F, seg=F, n_fine=13, c_in=64, c_out=32, w=F, bias=None, y=F, ld_y=32):
        return L.csn_octant_up_fwd_f32(x, ld_x, n_coarse, par, order, seg, n_fine, c_in, c_out, w, bias, y, ld_y, None)

    for f, idx in ((down, ("ch",)), (up, ("par", "order", "seg"))):
        for name in ("x", "w", "y") + idx:
            assert f(**{name: None}) == -1, name
        assert f(n_fine=0) == -1 and f(n_coarse=0) == -1
        assert f(c_in=40, ld_x=40) == -5 and f(c_in=288, ld_x=288) == -5 and f(c_in=0) == -5
        assert f(c_out=40, ld_y=40) == -5 and f(c_out=288, ld_y=288) == -5 and f(c_out=0) == -5
        assert f(ld_x=66) == -2 and f(ld_y=34) == -2
        assert f(ld_x=60) == -1 and f(ld_y=28) == -1                   # a row shorter than its channels
        assert f(x=F + 4) == -3 and f(y=F + 8) == -3 and f(w=F + 4) == -3
        for name in idx:
            assert f(**{name: F + 2}) == -3, name
    assert down(n_fine=1 << 24) == -5 and up(n_fine=1 << 24) == -5     # a map leaves the 2 GiB buffer window

    def down_b(dy=F, ld_dy=32, x=F, ld_x=64, n_fine=13, n_coarse=11, c_in=64, c_out=32, par=F, order=F, seg=F, w=F, dx=F, ld_dx=64,
               dw=F, db=F, ws_=F, wb=ws[0]):
        return L.csn_octant_down_bwd_f32(dy, ld_dy, x, ld_x, n_fine, n_coarse, c_in, c_out, par, order, seg, w, dx, ld_dx, dw, db, ws_,
                                         wb, None)

    def up_b(dy=F, ld_dy=32, x=F, ld_x=64, n_fine=13, n_coarse=11, c_in=64, c_out=32, ch=F, par=F, order=F, seg=F, w=F, dx=F, ld_dx=64,
             dw=F, db=F, ws_=F, wb=ws[1]):
        return L.csn_octant_up_bwd_f32(dy, ld_dy, x, ld_x, n_fine, n_coarse, c_in, c_out, ch, par, order, seg, w, dx, ld_dx, dw, db, ws_,
                                       wb, None)

    for f, idx in ((down_b, ("par", "order", "seg")), (up_b, ("ch", "par", "order", "seg"))):
        for name in ("dy", "ws_", "x", "w") + idx:
            assert f(**{name: None}) == -1, name
        assert f(n_fine=0) == -1 and f(n_coarse=0) == -1
        assert f(c_in=40, ld_x=40, ld_dx=40) == -5 and f(c_in=288, ld_x=288, ld_dx=288) == -5 and f(c_in=0) == -5
        assert f(c_out=40, ld_dy=40) == -5 and f(c_out=288, ld_dy=288) == -5 and f(c_out=0) == -5
        assert f(ld_dy=34) == -2 and f(ld_x=66) == -2 and f(ld_dx=66) == -2
        assert f(ld_dy=28) == -1 and f(ld_x=60) == -1 and f(ld_dx=60) == -1
        assert f(dy=F + 4) == -3 and f(dx=F + 4) == -3 and f(dw=F + 8) == -3 and f(ws_=F + 8) == -3 and f(x=F + 4) == -3
        for name in idx:
            assert f(**{name: F + 2}) == -3, name
        assert f(wb=f.__defaults__[-1] - 1) == -6
        # an output that is not asked for takes its own inputs with it
        assert f(dx=None, w=None, dw=None, x=None, db=None, wb=0) == -6


def test_the_abi_grew_by_five_exports_and_kept_its_version():
    import os
    import re
    from csn_amd import _lib
    _lib.build()
    new = {"csn_octant_conv_workspace_bytes", "csn_octant_down_fwd_f32", "csn_octant_down_bwd_f32", "csn_octant_up_fwd_f32",
           "csn_octant_up_bwd_f32"}
    assert new <= set(_lib.EXPORTS) and "octant_conv.hip" in _lib.SOURCES
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csn_hip.h")).read()
    assert re.search(r"#define CSN_ABI_VERSION 17\b", src)
    declared = set(re.findall(r"\b(csn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared == set(_lib.EXPORTS)                               # header <=> binding, as tests/test_cpu_abi.py holds it
    assert _lib.lib().csn_version() == 17


# ------------------------------------------------------------------------------------------------------
# modules and networks, host side
# ------------------------------------------------------------------------------------------------------
def test_modules_hold_minkowski_engine_names_and_refuse_the_wrong_map():
    from csn_amd import CsnError, SparseConvDown2, SparseConvUp2, build_kernel_map, build_octant_map, cat_conv3d, octant_conv_down
    down, up = SparseConvDown2(32, 64, bias=True), SparseConvUp2(64, 32)
    assert sorted(down.state_dict()) == ["bias", "kernel"] and down.kernel.shape == (8, 32, 64) and down.bias.shape == (1, 64)
    assert list(up.state_dict()) == ["kernel"] and up.kernel.shape == (8, 64, 32)
    assert "kernel_size=2, stride=2" in repr(down) and abs(float(down.kernel.detach().std()) - (8 * 32) ** -0.5) < 0.01
    for bad in (dict(c_in=3, c_out=32), dict(c_in=32, c_out=40), dict(c_in=288, c_out=32), dict(c_in=32, c_out=0)):
        with pytest.raises(ValueError):
            SparseConvDown2(**bad)
    coords = torch.tensor(R.dense_block())
    om, km = build_octant_map(coords), build_kernel_map(coords, 3, stride=2)
    xf, xc = torch.zeros(om.n_fine, 32), torch.zeros(om.n_coarse, 64)
    for layer, x, m in ((down, xf, km), (up, xc, km.transpose()), (down, xc[:, :32], om), (up, torch.zeros(om.n_fine, 64), om)):
        with pytest.raises(ValueError):
            layer(x, m)
    for layer, x in ((down, xf), (up, xc)):
        with pytest.raises(CsnError):
            layer(x, om)
    with pytest.raises(CsnError):
        octant_conv_down(xf, down.kernel, None, om)
    with pytest.raises(ValueError):
        cat_conv3d([xf, xf], torch.zeros(27, 96, 32), build_kernel_map(coords, 3))


# the reference's state_dict of Res16UNet14A, written out from res16unet.py:24-175 (LAYERS all 1; block1 keeps its width: no downsample)
_BN = ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked")
_14A_CONVS = ("conv0p1s1", "conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2", "convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")
_14A_NORMS = ("bn0", "bn1", "bn2", "bn3", "bn4", "bntr4", "bntr5", "bntr6", "bntr7")
RES16UNET14A_KEYS = sorted(
    [f"{c}.kernel" for c in _14A_CONVS] + [f"{n}.{q}" for n in _14A_NORMS for q in _BN]
    + [f"block{b}.0.{c}.kernel" for b in range(1, 9) for c in ("conv1", "conv2")]
    + [f"block{b}.0.{n}.{q}" for b in range(1, 9) for n in ("norm1", "norm2") for q in _BN]
    + [f"block{b}.0.downsample.0.kernel" for b in range(2, 9)] + [f"block{b}.0.downsample.1.{q}" for b in range(2, 9) for q in _BN]
    + ["final.kernel", "final.bias"])


def test_classes_construct_with_the_reference_key_set_and_the_refused_ones_raise():
    import csn_amd
    from csn_amd import minkowski_unet as MU
    assert len(MU.SUPPORTED) == 14
    for name in MU.SUPPORTED:
        model = getattr(csn_amd, name)(3, 6)
        assert isinstance(model, csn_amd.Res16UNetBase) and model.final.out_features == 6 and model.bn0.momentum == 0.02
        if name in U.NETS:
            shapes = U.param_shapes(name)
            assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes
            assert (model.PLANES, model.LAYERS) == U.NETS[name]
    assert sorted(U.me_keys(csn_amd.Res16UNet14A(3, 6).state_dict())) == RES16UNET14A_KEYS
    # Res16UNet14: every decoder block reads more than 256 columns; Res16UNet14A: none does
    wide = lambda m: [isinstance(getattr(m, f"block{b}")[0].conv1, MU.CatConv3d) for b in range(5, 9)]
    assert wide(csn_amd.Res16UNet14(3, 6)) == [True] * 4 and wide(csn_amd.Res16UNet14A(3, 6)) == [False] * 4
    for name, word in (("Res16UNet14D", "384"), ("Res16UNet18D", "384"), ("Res16UNet50", "Bottleneck"), ("Res16UNet101", "Bottleneck")):
        with pytest.raises(NotImplementedError, match=word):
            getattr(csn_amd, name)(3, 6)

    class LayerNormNet(csn_amd.Res16UNet14A):
        NORM_TYPE = "LAYER_NORM"
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        LayerNormNet(3, 6)
    with pytest.raises(csn_amd.CsnError):
        csn_amd.Res16UNet14A(3, 6)((torch.tensor(R.random_set(300)), torch.zeros(300, 3)))


def test_load_me_unet_state_round_trips_the_reference_layout():
    from csn_amd import Res16UNet14A, load_me_unet_state
    from csn_amd.minkowski_trainer import checkpoint_num_labels, load_model_state
    p = U.params("Res16UNet14A")
    ref = {}
    for own, there in zip(p, U.me_keys(p)):
        v = p[own]
        if own == "final.weight":
            v = v.t()[None]                                            # (1, c, out)
        elif own == "final.bias":
            v = v[None]                                                # (1, out)
        ref[there] = v.clone()
    assert sorted(ref) == RES16UNET14A_KEYS and checkpoint_num_labels(ref) == 6 and checkpoint_num_labels(p) == 6
    model = load_me_unet_state(Res16UNet14A(3, 6), ref)
    for k, v in model.state_dict().items():
        assert torch.equal(v, p[k]), k
    other = Res16UNet14A(3, 6)
    load_model_state(other, ref)                                       # the trainer's loader finds the layout ...
    load_model_state(other, model.state_dict())                        # ... and this project's own
    assert torch.equal(other.block5[0].downsample[0].kernel, p["block5.0.downsample.0.kernel"])
    flat = dict(ref)
    flat["block2.0.downsample.0.kernel"] = ref["block2.0.downsample.0.kernel"][0]      # a kernel-1 convolution kept as (c_in, c_out)
    flat["final.kernel"], flat["final.bias"] = ref["final.kernel"][0], ref["final.bias"][0]
    load_me_unet_state(Res16UNet14A(3, 6), flat)
    for name, bad in (("conv1p1s2.kernel", torch.zeros(27, 32, 32)), ("final.kernel", torch.zeros(1, 96, 7)),
                      ("bn0.bn.weight", torch.zeros(64))):
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            load_me_unet_state(Res16UNet14A(3, 6), {**ref, name: bad})
    with pytest.raises(ValueError, match="no bntr7"):
        load_me_unet_state(Res16UNet14A(3, 6), {k: v for k, v in ref.items() if k != "bntr7.bn.bias"})


def test_unet_pyramid_levels_are_build_pyramids():
    from csn_amd import build_pyramid, build_unet_pyramid
    coords = torch.tensor(R.random_set(300))
    u, h = build_unet_pyramid(coords), build_pyramid(coords, 5)
    assert len(u.coords) == 5 and len(u.oct) == 4 and u.stem.kernel_size == 5 and build_unet_pyramid(coords, 3).stem is not None
    for l in range(5):
        assert torch.equal(u.coords[l], h.coords[l]) and torch.equal(u.s1[l].fwd, h.s1[l].fwd)
        assert u.one[l].kernel_size == 1 and u.one[l].fwd.tolist() == [list(range(u.coords[l].shape[0]))]
        if l < 4:
            assert (u.oct[l].in_tensor_stride, u.oct[l].n_fine, u.oct[l].n_coarse) == (1 << l, u.coords[l].shape[0], u.coords[l + 1].shape[0])
    assert u.to("cpu").oct[0].seg.tolist() == u.oct[0].seg.tolist()


def test_train_seg_parser_takes_the_supported_unets():
    from csn_amd import minkowski_unet as MU
    from csn_amd import train_csn, train_seg
    assert set(MU.SUPPORTED) <= set(train_seg.MODELS) and not set(MU.REFUSED) & set(train_seg.MODELS)
    assert train_seg.parse_args(["--synthetic", "6", "--model", "Res16UNet34C"])[0].model == "Res16UNet34C"
    for module, bad in ((train_seg, "Res16UNet14D"), (train_seg, "Res16UNet50"), (train_csn, "Res16UNet34C")):
        with pytest.raises(SystemExit):
            module.parse_args(["--synthetic", "6", "--model", bad])
