"""Point fields on the MI355X (csn_amd.minkowski_field, include/csn_hip.h section 16) against the float64 restatement of
tests/field_ref.py.  Bounds are computed, not chosen (u = 2^-24, the unit roundoff of fp32):

  forward   |err| <= 2^-20 sum_c w_c |z_c| + 1e-30    at most 13 roundings on the path of one term and the eight-term sum
  backward  |err| <= (n_v + 8) u sum w |dy| + 1e-30   n_v the (point, corner) contributions of the voxel, added one after the other
  average   |err| <= (n + 2) u mean |f| + 1e-30       n the points of the voxel

Every test prints its worst error / bound (``[field] ...`` under ``pytest -s``)."""
import functools

import numpy as np
import pytest
import torch

from tests import field_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
U = 2.0 ** -24
WIDTHS = [1, 3, 39, 64, 65, 256]
LAYOUTS = ["natural", "block4", "block1"]      # contiguous; a 16-byte aligned column block at a pitch % 4 == 0; an odd block at an odd pitch
SETS = ["n1", "n63", "n65", "n1031", "isolated", "full_block", "shared_xyz", "lattice", "range_edge", "heavy_voxel"]


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _points(name):
    coords = R.random_points(int(name[1:]), seed=int(name[1:])) if name[0] == "n" and name[1:].isdigit() else R.special_sets()[name]
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    return coords, R.quantise(coords, np.zeros((coords.shape[0], 1)))


@functools.lru_cache(maxsize=None)
def _field(name):
    from csn_amd import PointField
    coords, _ = _points(name)
    return PointField(torch.from_numpy(coords).cuda(), torch.zeros(coords.shape[0], 1, device="cuda"))


def _block(values, layout):
    """``values (n, C)`` as a device tensor in the layout: (view, whole buffer)."""
    n, c = values.shape
    if layout == "natural":
        t = values.cuda().contiguous()
        return t, t
    off, pitch = (4, (c + 4 + 5 + 3) // 4 * 4) if layout == "block4" else (1, c + 3 + (c % 2 == 1))
    buf = torch.full((n, pitch), CANARY, device="cuda")
    view = buf[:, off:off + c]
    view.copy_(values)
    return view, buf


def _intact(view, buf, c):
    if view is buf:
        return True
    off = view.storage_offset() - buf.storage_offset()
    mask = torch.ones(buf.shape[1], dtype=torch.bool, device="cuda")
    mask[off:off + c] = False
    return bool((buf[:, mask] == CANARY).all())


@pytest.mark.parametrize("name", SETS)
def test_interpolation_forward_and_backward(L, name):
    from csn_amd.minkowski_field import interpolate_rows, interpolate_rows_backward
    coords, q = _points(name)
    f = _field(name)
    assert np.array_equal(f.voxel_coords.cpu().numpy(), q["voxel_coords"]) and np.array_equal(f.home.cpu().numpy(), q["home"])
    assert np.array_equal(f.vox_ptr.cpu().numpy(), q["vox_ptr"]) and np.array_equal(f.vox_pts.cpu().numpy(), q["vox_pts"])
    if name == "isolated":
        assert (f.corner_table()[[14, 16, 17, 22, 23, 25, 26]] < 0).all()
    if name == "range_edge":
        assert int((f.corner_table()[14] >= 0).sum()) == 1                  # floor + 1 leaves the packed range: "no voxel"
    if name == "heavy_voxel":
        assert q["counts"].max() == 300 and np.median(q["counts"]) == 1
    n_pts, n_vox = coords.shape[0], q["voxel_coords"].shape[0]
    table = f.corner_table()
    worst_f = worst_b = 0.0
    for c in WIDTHS:
        g = torch.Generator().manual_seed(1000 + c)
        z = torch.randn(n_vox, c, generator=g)
        dy = torch.randn(n_pts, c, generator=g)
        y_ref, y_scale = R.interpolate(coords, q["voxel_coords"], z.numpy())
        dz_ref, dz_scale, n_v = R.adjoint(coords, q["voxel_coords"], dy.numpy())
        for layout in LAYOUTS:
            zv, _ = _block(z, layout)
            yv, ybuf = _block(torch.full((n_pts, c), CANARY), layout)
            interpolate_rows(zv, f.coords, f.home, table, out=yv)
            err = np.abs(yv.cpu().numpy().astype(np.float64) - y_ref)
            bound = 2.0 ** -20 * y_scale + 1e-30
            worst_f = max(worst_f, float((err / bound).max()))
            assert (err <= bound).all(), (name, c, layout, "forward", float((err / bound).max()))
            assert _intact(yv, ybuf, c), (name, c, layout, "forward wrote outside its columns")

            dyv, _ = _block(dy, layout)
            dzv, dzbuf = _block(torch.full((n_vox, c), CANARY), layout)
            interpolate_rows_backward(dyv, f.coords, f.vox_ptr, f.vox_pts, table, out=dzv)
            got = dzv.clone()
            err = np.abs(got.cpu().numpy().astype(np.float64) - dz_ref)               # (every row is written: no canary is left)
            bound = (n_v[:, None] + 8) * U * dz_scale + 1e-30
            worst_b = max(worst_b, float((err / bound).max()))
            assert (err <= bound).all(), (name, c, layout, "backward", float((err / bound).max()))
            assert _intact(dzv, dzbuf, c), (name, c, layout, "backward wrote outside its columns")
            dzv.fill_(CANARY)
            interpolate_rows_backward(dyv, f.coords, f.vox_ptr, f.vox_pts, table, out=dzv)
            assert torch.equal(dzv, got), (name, c, layout, "two backward calls differ")
    print(f"[field] {name}: {n_pts} points, {n_vox} voxels: forward err / bound {worst_f:.3f}, backward err / bound {worst_b:.3f}")


@pytest.mark.parametrize("name", ["n63", "n1031", "shared_xyz", "heavy_voxel"])
def test_voxel_average(L, name):
    from csn_amd import PointField
    from csn_amd.minkowski_field import voxel_mean
    coords, _ = _points(name)
    worst = 0.0
    for cf in (1, 3, 64):
        g = torch.Generator().manual_seed(cf)
        feats = torch.randn(coords.shape[0], cf, generator=g)
        q = R.quantise(coords, feats.numpy())
        bound = (q["counts"][:, None] + 2) * U * q["mean_abs"] + 1e-30
        f = PointField(torch.from_numpy(coords).cuda(), feats.cuda(), "unweighted_average")
        where, vf = f.sparse()
        err = np.abs(vf.cpu().numpy().astype(np.float64) - q["mean"])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (name, cf, float((err / bound).max()))
        fv, _ = _block(feats, "block1")                                      # the features as a column block: any pitch
        assert torch.equal(voxel_mean(fv, f.vox_ptr, f.vox_pts), vf)
        # the output at a pitch of its own, through the C ABI
        out = torch.full((f.n_voxels, cf + 3), CANARY, device="cuda")
        L.check(L.lib().csn_voxel_mean_f32(fv.data_ptr(), fv.stride(0), f.n_points, f.vox_ptr.data_ptr(), f.vox_pts.data_ptr(), f.n_voxels,
                                           cf, out.data_ptr(), cf + 3, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(out[:, :cf], vf) and bool((out[:, cf:] == CANARY).all())
        first = PointField(torch.from_numpy(coords).cuda(), feats.cuda()).sparse()[1]
        assert np.array_equal(first.cpu().numpy(), q["first"].astype(np.float32))
    print(f"[field] {name}: average err / bound {worst:.3f}")


def test_autograd_node_and_the_skipped_gradient(L):
    coords, q = _points("n65")
    f = _field("n65")
    calls = []
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    try:
        z = torch.randn(f.n_voxels, 39, device="cuda", requires_grad=True)
        dy = torch.randn(f.n_points, 39, device="cuda")
        y = f.interpolate(z)
        y.backward(dy)
        assert calls == ["csn_point_interp_fwd_f32", "csn_point_interp_bwd_f32"]
        dz_ref, dz_scale, n_v = R.adjoint(coords, q["voxel_coords"], dy.cpu().numpy())
        assert (np.abs(z.grad.cpu().numpy().astype(np.float64) - dz_ref) <= (n_v[:, None] + 8) * U * dz_scale + 1e-30).all()
        # z needs no gradient: the backward pass of the graph around the node launches nothing of section 16
        del calls[:]
        s = torch.ones((), device="cuda", requires_grad=True)
        y = f.interpolate(z.detach()) * s
        y.backward(dy)
        assert s.grad is not None and calls == ["csn_point_interp_fwd_f32"]
    finally:
        L.set_call_hook(None)


def test_cpu_tensors_raise(L):
    from csn_amd import CsnError, PointField
    from csn_amd.minkowski_field import voxel_mean
    coords, _ = _points("n63")
    dev, host = _field("n63"), PointField(torch.from_numpy(coords), torch.zeros(coords.shape[0], 1))
    with pytest.raises(CsnError):
        dev.interpolate(torch.zeros(dev.n_voxels, 4))
    with pytest.raises(CsnError):
        host.interpolate(torch.zeros(host.n_voxels, 4, device="cuda"))
    with pytest.raises(CsnError):
        dev.interpolate(torch.zeros(dev.n_voxels, 4, device="cuda", dtype=torch.float64))
    with pytest.raises(CsnError):
        voxel_mean(torch.zeros(coords.shape[0], 2), host.vox_ptr, host.vox_pts)
    moved = host.to("cuda")
    z = torch.randn(dev.n_voxels, 4, device="cuda")
    assert torch.equal(moved.interpolate(z), dev.interpolate(z))


def test_end_to_end_with_hrnet_simcsn2s(L):
    """Points -> voxel rows -> HRNetSimCSN2S -> point logits -> seg_loss, and one train_iter on per-point targets."""
    from csn_amd import HRNetSimCSN2S, PointField, batch_points, seg_loss, train_iter
    torch.manual_seed(7)
    rng = np.random.default_rng(7)
    shapes = [(torch.from_numpy(rng.normal(scale=0.1, size=(n, 3))), torch.randn(n, 3), torch.from_numpy(rng.integers(0, 6, size=n)))
              for n in (150, 147)]
    coords, feats, target = batch_points(shapes, 0.05)
    field = PointField(coords.cuda(), feats.cuda())
    assert field.offsets.tolist() == [0, 150, 297] and 50 < field.n_voxels < 297
    model = HRNetSimCSN2S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().train()
    field.pyramid(2)
    vlog = model(field.sparse())
    vlog.retain_grad()
    plog = field.interpolate(vlog)
    plog.retain_grad()
    assert plog.shape == (297, 6)
    loss, _ = seg_loss(plog, target.cuda(), field.offsets)
    loss.backward()
    c_np, vc = coords.numpy(), field.voxel_coords.cpu().numpy()
    y_ref, y_scale = R.interpolate(c_np, vc, vlog.detach().cpu().numpy())
    assert (np.abs(plog.detach().cpu().numpy().astype(np.float64) - y_ref) <= 2.0 ** -20 * y_scale + 1e-30).all()
    dz_ref, dz_scale, n_v = R.adjoint(c_np, vc, plog.grad.cpu().numpy())
    assert float(np.abs(dz_ref).max()) > 0
    assert (np.abs(vlog.grad.cpu().numpy().astype(np.float64) - dz_ref) <= (n_v[:, None] + 8) * U * dz_scale + 1e-30).all()

    forward_fn = lambda fld: (fld.interpolate(model(fld.sparse())), fld.offsets)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    batch_loss, prec = train_iter(forward_fn, [(field, target)], opt)
    assert bool(torch.isfinite(batch_loss)) and bool(torch.isfinite(prec))
    changed = sum(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    assert changed > len(before) // 2                                       # (linear_q / linear_k see no key batch)
