"""Sparse 3D convolution on voxel rows (csn_amd/minkowski_conv.py, csn_amd/csrc/sparse_conv.hip, include/csn_hip.h section 14),
without a GPU: the float64 restatement tests/sparse_conv_ref.py against torch's dense conv3d / conv_transpose3d, its gradients
against autograd, ``build_kernel_map`` on CPU tensors against the coordinate dictionary, the host-side argument checks of the raw
ABI, the modules' parameters, and the share of undecided ReLU pre-activations of the block case the GPU test uses."""
import pytest
import torch
import torch.nn.functional as F

from tests import sparse_conv_ref as R

TS = 2                                   # the dense checks run at tensor stride 2: offsets step by 2


def _points(n=None):
    """2 shapes on a 12^3 grid at tensor stride TS, negative coordinates included."""
    return R.random_set(n, ts=TS, seed=1)


def _dense(coords, x, lo, side, step):
    """Scatter rows onto a (B, C, Z, Y, X) grid; coordinate c sits at (c - lo) / step."""
    B = max(c[0] for c in coords) + 1
    vol = torch.zeros(B, x.shape[1], side, side, side, dtype=torch.float64)
    for row, (b, cx, cy, cz) in zip(x, coords):
        vol[b, :, (cz - lo) // step, (cy - lo) // step, (cx - lo) // step] = row
    return vol


def _sample(vol, coords, lo, step):
    return torch.stack([vol[b, :, (cz - lo) // step, (cy - lo) // step, (cx - lo) // step] for b, cx, cy, cz in coords])


def _dense_weight(w, k, transposed=False):
    """(KV, c_in, c_out) -> conv3d's (c_out, c_in, z, y, x) or conv_transpose3d's (c_in, c_out, z, y, x)."""
    v = w.double().view(k, k, k, w.shape[1], w.shape[2])                 # (z, y, x, c_in, c_out): x fastest in kidx
    return v.permute(3, 4, 0, 1, 2) if transposed else v.permute(4, 3, 0, 1, 2)


@pytest.mark.parametrize("k", [3, 5])
def test_stride_1_equals_dense_conv3d(k):
    coords = _points()
    g, out = R.geometry("s1", coords, k=k, ts=TS)
    t = R.tensors(1, len(coords), len(out), k ** 3, 8, 16)
    lo, side = -12, 12
    y = R.fwd(g, t["x"], t["w"], t["b"])
    dense = F.conv3d(_dense(out, t["x"].double(), lo, side, TS), _dense_weight(t["w"], k), t["b"].double(), padding=k // 2)
    assert (y - _sample(dense, out, lo, TS)).abs().max() < 1e-12


def test_stride_2_equals_dense_conv3d():
    coords = _points()
    g, out = R.geometry("s2", coords, ts=TS)
    assert all(v % (2 * TS) == 0 for c in out for v in c[1:]) and out == sorted(out)
    t = R.tensors(2, len(coords), len(out), 27, 8, 16)
    lo, side = -12, 12
    y = R.fwd(g, t["x"], t["w"])
    dense = F.conv3d(_dense([tuple(c) for c in coords], t["x"].double(), lo, side, TS), _dense_weight(t["w"], 3), stride=2, padding=1)
    assert (y - _sample(dense, out, lo, 2 * TS)).abs().max() < 1e-12


def test_transposed_equals_dense_conv_transpose3d():
    fine = _points()
    coarse = R.down_coords([tuple(c) for c in fine], TS)
    g, out = R.geometry("tr", coarse, ts=TS, fine=fine)
    t = R.tensors(3, len(coarse), len(fine), 27, 8, 16)
    lo = -12
    y = R.fwd(g, t["x"], t["w"])
    dense = F.conv_transpose3d(_dense(coarse, t["x"].double(), lo, 6, 2 * TS), _dense_weight(t["w"], 3, transposed=True), stride=2,
                               padding=1, output_padding=1)
    assert (y - _sample(dense, out, lo, TS)).abs().max() < 1e-12
    # adjoint identity: <down(x; W), g> = <x, up(g; W^T)>
    gd, _ = R.geometry("s2", fine, ts=TS)
    xf, gc = R.tensors(4, len(fine), len(coarse), 27, 8, 16)["x"], R.tensors(5, len(coarse), 1, 1, 16, 1)["x"]
    w = t["w"]
    lhs = (R.fwd(gd, xf, w) * gc.double()).sum()
    rhs = (xf.double() * R.fwd(g, gc, w.transpose(1, 2))).sum()
    assert abs(lhs - rhs) < 1e-10 * max(1.0, abs(lhs))


@pytest.mark.parametrize("mode", ["s1", "s2", "tr"])
def test_restated_gradients_equal_autograd(mode):
    fine = _points(129)
    coarse = R.down_coords([tuple(c) for c in fine], TS)
    g, out = R.geometry(mode, coarse if mode == "tr" else fine, ts=TS, fine=fine)
    t = R.tensors(6, g.n_in, g.n_out, 27, 8, 16)
    x, w, b = (t[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    (( R._conv_autograd(g, x, w) + b) * t["dy"].double()).sum().backward()
    got = R.bwd(g, t["dy"], t["x"], t["w"])
    assert (got["dx"] - x.grad).abs().max() < 1e-12 and (got["dw"] - w.grad).abs().max() < 1e-12
    assert (got["dbias"] - b.grad).abs().max() < 1e-12
    assert got["scale_dx"] >= got["dx"].abs().max() and got["scale_dw"] >= got["dw"].abs().max()


# ------------------------------------------------------------------------------------------------------
# build_kernel_map
# ------------------------------------------------------------------------------------------------------
def _tables_from(g):
    """fwd (KV, n_out) / bwd (KV, n_in) of a dictionary geometry."""
    fwd = torch.full((g.KV, g.n_out), -1, dtype=torch.int32)
    bwd = torch.full((g.KV, g.n_in), -1, dtype=torch.int32)
    for kidx, (j, i) in enumerate(g.pairs):
        fwd[kidx, j] = i.int()
        bwd[kidx, i] = j.int()
    return fwd, bwd


@pytest.mark.parametrize("k", [3, 5])
def test_map_stride_1_agrees_with_the_dictionary(k):
    from csn_amd.minkowski_conv import build_kernel_map
    coords = _points()
    g, _ = R.geometry("s1", coords, k=k, ts=TS)
    m = build_kernel_map(torch.tensor(coords), kernel_size=k, tensor_stride=TS)
    fwd, bwd = _tables_from(g)
    assert m.fwd.dtype == torch.int32 and m.fwd.shape == (k ** 3, len(coords)) and m.fwd.is_contiguous()
    assert torch.equal(m.fwd, fwd) and torch.equal(m.bwd, bwd)
    assert m.bwd_table is None                                          # no second table: the kernel walks fwd in reversed order
    for kidx in range(k ** 3):
        assert torch.equal(m.bwd[kidx], m.fwd[k ** 3 - 1 - kidx])
    assert m.out_tensor_stride == TS and torch.equal(m.out_coords, torch.tensor(coords)) and m.KV == k ** 3
    centre = k ** 3 // 2
    assert torch.equal(m.fwd[centre], torch.arange(len(coords), dtype=torch.int32))


def test_map_stride_2_and_transpose_agree_with_the_dictionary():
    from csn_amd.minkowski_conv import build_kernel_map
    fine = _points()
    g, out = R.geometry("s2", fine, ts=TS)
    m = build_kernel_map(torch.tensor(fine), kernel_size=3, stride=2, tensor_stride=TS)
    fwd, bwd = _tables_from(g)
    assert m.out_tensor_stride == 2 * TS and m.out_coords.tolist() == [list(c) for c in out]
    assert torch.equal(m.fwd, fwd) and torch.equal(m.bwd, bwd)
    # the transposed convolution's map is the same two tables, swapped
    gt, _ = R.geometry("tr", out, ts=TS, fine=fine)
    tf, tb = _tables_from(gt)
    up = m.transpose()
    assert up.transposed and up.stride == 2 and up.out_tensor_stride == TS and up.n_in == len(out) and up.n_out == len(fine)
    assert up.fwd is m.bwd and up.bwd is m.fwd
    assert torch.equal(up.fwd, tf) and torch.equal(up.bwd, tb)
    assert up.transpose().fwd is m.fwd and not up.transpose().transposed
    # ... and equals a transposed map built on its own, onto the given fine set
    own = build_kernel_map(m.out_coords, kernel_size=3, stride=2, tensor_stride=2 * TS, out_coords=torch.tensor(fine), transposed=True)
    assert torch.equal(own.fwd, tf) and torch.equal(own.bwd, tb) and own.out_tensor_stride == TS


def test_map_never_crosses_batch_indices():
    from csn_amd.minkowski_conv import build_kernel_map
    one = R.dense_block()
    coords = torch.tensor(one + [[1] + c[1:] for c in one])            # identical xyz, different b
    n = len(one)
    for stride in (1, 2):
        m = build_kernel_map(coords, kernel_size=3, stride=stride)
        ob = m.out_coords[:, 0]
        for table, src_b, dst_b in ((m.fwd, coords[:, 0], ob), (m.bwd, ob, coords[:, 0])):
            hit = table >= 0
            assert bool(hit.any())
            assert torch.equal(src_b[table.long().clamp(min=0)][hit], dst_b.expand_as(table)[hit])
    assert int((build_kernel_map(coords, 3).fwd >= 0).sum()) == 2 * int((build_kernel_map(coords[:n], 3).fwd >= 0).sum())


def test_map_floors_negative_coordinates():
    from csn_amd.minkowski_conv import build_kernel_map
    coords = torch.tensor([[0, -1, -2, -3], [0, 1, 0, -4], [0, -5, 3, 2]])
    m = build_kernel_map(coords, kernel_size=3, stride=2)
    assert m.out_coords.tolist() == [[0, -6, 2, 2], [0, -2, -2, -4], [0, 0, 0, -4]]       # floor: -1 -> -2, -3 -> -4, -5 -> -6
    # (0, -1, -2, -3) = (0, -2, -2, -4) + (1, 0, 1): kidx = 2 + 3 * 1 + 9 * 2
    assert m.fwd[2 + 3 + 18, 1] == 0 and m.bwd[2 + 3 + 18, 0] == 1


def test_map_refuses_what_it_does_not_take():
    from csn_amd.minkowski_conv import build_kernel_map
    ok = torch.tensor([[0, 0, 0, 0], [0, 2, 0, 0]])
    build_kernel_map(ok, 3, 1, 2)
    bad = [dict(coords=torch.tensor([[1 << 15, 0, 0, 0]])), dict(coords=torch.tensor([[-1, 0, 0, 0]])),
           dict(coords=torch.tensor([[0, 1 << 15, 0, 0]])), dict(coords=torch.tensor([[0, 0, -(1 << 15) - 1, 0]])),
           dict(coords=torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3]])),                        # duplicate rows
           dict(coords=torch.tensor([[0, 1, 0, 0]]), tensor_stride=2),                     # not a multiple of the tensor stride
           dict(coords=ok, kernel_size=2), dict(coords=ok, kernel_size=4), dict(coords=ok, stride=3), dict(coords=ok, stride=0),
           dict(coords=ok, stride=2, kernel_size=5),
           dict(coords=ok, stride=2, tensor_stride=2, transposed=True),                    # transposed without out_coords
           dict(coords=ok, stride=2, tensor_stride=2, transposed=True, out_coords=torch.tensor([[0, 1, 1, 1], [0, 1, 1, 1]])),
           dict(coords=torch.zeros(0, 4, dtype=torch.long)), dict(coords=torch.zeros(3, 3, dtype=torch.long))]
    for kw in bad:
        with pytest.raises(ValueError):
            build_kernel_map(**kw)
    # the extremes of the packed range are taken, and their neighbours beyond it are "no voxel", not a wrapped key
    edge = torch.tensor([[(1 << 15) - 1, (1 << 15) - 1, -(1 << 15), 0], [0, -(1 << 15), (1 << 15) - 1, 0]])
    m = build_kernel_map(edge, 3)
    assert int((m.fwd >= 0).sum()) == 2


# ------------------------------------------------------------------------------------------------------
# raw ABI and modules, host side
# ------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    FAKE = 1 << 20
    ws_b = L.csn_sparse_conv_workspace_bytes(13, 11, 27, 64, 32, 1)
    assert ws_b > 0 and L.csn_sparse_conv_workspace_bytes(13, 11, 27, 64, 32, 0) == 0
    assert L.csn_sparse_conv_workspace_bytes(13, 11, 8, 64, 32, 1) == 0 and L.csn_sparse_conv_workspace_bytes(0, 11, 27, 64, 32, 1) == 0

    def fwd(x=FAKE, ld_x=64, n_in=13, table=FAKE, n_out=11, kv=27, c_in=64, c_out=32, w=FAKE, bias=None, y=FAKE, ld_y=32):
        return L.csn_sparse_conv_fwd_f32(x, ld_x, n_in, table, n_out, kv, c_in, c_out, w, bias, y, ld_y, None)
    assert fwd(x=None) == -1 and fwd(table=None) == -1 and fwd(w=None) == -1 and fwd(y=None) == -1
    assert fwd(n_in=0) == -1 and fwd(n_out=0) == -1
    assert fwd(kv=8) == -5 and fwd(kv=343) == -5
    assert fwd(c_in=40, ld_x=40) == -5 and fwd(c_out=48, ld_y=48) == -5 and fwd(c_in=288, ld_x=288) == -5 and fwd(c_out=0) == -5
    assert fwd(ld_x=66) == -2 and fwd(ld_y=34) == -2
    assert fwd(ld_x=60) == -1 and fwd(ld_y=28) == -1                  # a row shorter than its channels
    assert fwd(x=FAKE + 4) == -3 and fwd(y=FAKE + 8) == -3 and fwd(w=FAKE + 4) == -3 and fwd(table=FAKE + 2) == -3
    assert fwd(n_in=1 << 24, ld_x=64) == -5                           # the gathered map leaves the 2 GiB buffer window

    def bwd(dy=FAKE, ld_dy=32, x=FAKE, ld_x=64, n_in=13, n_out=11, kv=27, c_in=64, c_out=32, ft=FAKE, bt=FAKE, w=FAKE, dx=FAKE,
            ld_dx=64, dw=FAKE, db=FAKE, ws=FAKE, wb=ws_b):
        return L.csn_sparse_conv_bwd_f32(dy, ld_dy, x, ld_x, n_in, n_out, kv, c_in, c_out, ft, bt, w, dx, ld_dx, dw, db, ws, wb, None)
    assert bwd(dy=None) == -1 and bwd(ws=None) == -1 and bwd(bt=None) == -1 and bwd(w=None) == -1 and bwd(ft=None) == -1
    assert bwd(x=None) == -1
    assert bwd(bt=None, ft=None, n_in=11) == -1                        # the stride-1 identity needs the forward table (and n_in == n_out)
    assert bwd(n_in=0) == -1 and bwd(kv=9) == -5 and bwd(c_in=40, ld_x=40, ld_dx=40) == -5 and bwd(c_out=48, ld_dy=48) == -5
    assert bwd(ld_dy=34) == -2 and bwd(ld_x=66) == -2 and bwd(ld_dx=66) == -2
    assert bwd(ld_dy=28) == -1 and bwd(ld_dx=60) == -1
    assert bwd(dy=FAKE + 4) == -3 and bwd(dx=FAKE + 4) == -3 and bwd(dw=FAKE + 8) == -3 and bwd(ws=FAKE + 8) == -3
    assert bwd(wb=ws_b - 1) == -6


def test_modules_hold_minkowski_engine_names_and_refuse_the_wrong_map():
    from csn_amd import CsnError, SparseBasicBlock, SparseConv3d, SparseConvTranspose3d, build_kernel_map, sparse_conv3d
    stem = SparseConv3d(3, 32, kernel_size=5)
    assert list(stem.state_dict()) == ["kernel"] and stem.kernel.shape == (125, 3, 32)
    down = SparseConv3d(64, 128, kernel_size=3, stride=2, bias=True)
    assert sorted(down.state_dict()) == ["bias", "kernel"] and down.kernel.shape == (27, 64, 128) and down.bias.shape == (1, 128)
    up = SparseConvTranspose3d(128, 64)
    assert up.kernel.shape == (27, 128, 64) and up.bias is None
    blk = SparseBasicBlock(64, 64)
    assert sorted(n for n, _ in blk.named_parameters()) == ["conv1.kernel", "conv2.kernel", "norm1.bias", "norm1.weight", "norm2.bias",
                                                            "norm2.weight"]
    assert blk.norm1.momentum == 0.02 and blk.downsample is None and isinstance(blk.norm2, torch.nn.BatchNorm1d)
    for bad in (dict(c_in=3, c_out=33), dict(c_in=300, c_out=32), dict(c_in=32, c_out=32, kernel_size=4),
                dict(c_in=32, c_out=32, kernel_size=5, stride=2), dict(c_in=32, c_out=32, stride=3)):
        with pytest.raises(ValueError):
            SparseConv3d(**bad)
    coords = torch.tensor(R.dense_block())
    m1, m5, m2 = build_kernel_map(coords, 3), build_kernel_map(coords, 5), build_kernel_map(coords, 3, stride=2)
    x3, x64, xc = torch.zeros(64, 3), torch.zeros(64, 64), torch.zeros(m2.n_out, 128)
    for layer, x, m in ((stem, x3, m1), (down, x64, m1), (down, x64, m2.transpose()), (up, xc, m2), (up, xc, m1),
                        (blk.conv1, x64, m5), (blk.conv1, x64, m2)):
        with pytest.raises(ValueError):
            layer(x, m)
    # the right map on CPU rows: no CPU path
    for layer, x, m in ((stem, x3, m5), (down, x64, m2), (up, xc, m2.transpose()), (blk, x64, m1)):
        with pytest.raises(CsnError):
            layer(x, m)
    with pytest.raises(CsnError):
        sparse_conv3d(x64, blk.conv1.kernel, None, m1)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_block_case_has_decided_relu_masks(training):
    """The GPU test compares the block's outputs and masks where the float64 pre-activation is at least 1e-4 from zero; at most
    0.1 % of the elements may be nearer (about 0.008 % expected for unit-variance batch-norm outputs).  Asserted here, on the
    reference alone."""
    coords, p, x, _ = R.block_case()
    g, _ = R.geometry("s1", coords)
    _, a1, a2 = R.block(g, x.double(), {k: v.double() for k, v in p.items()}, training)
    for a in (a1, a2):
        share = (a.abs() < 1e-4).double().mean().item()
        print(f"[sparse_conv] block {'train' if training else 'eval'}: undecided {share:.2e}")
        assert share <= 1e-3
