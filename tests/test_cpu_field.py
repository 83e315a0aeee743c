"""Point fields without a GPU (csn_amd.minkowski_field, include/csn_hip.h section 16): the float64 restatement of tests/field_ref.py
against torch's ``grid_sample`` on the dense volume, its own identities, and ``PointField``'s plumbing on CPU tensors against the
restatement; argument validation of the field and, on the host, of the three raw entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import field_ref as R


def _dense_check(coords, voxel_coords, z):
    """max |restatement - grid_sample| over the points, shape by shape, on the dense volume that holds the voxel set."""
    coords = np.asarray(coords, dtype=np.float32)
    vc = np.asarray(voxel_coords)
    y, _ = R.interpolate(coords, vc, z, exact_t=True)
    worst = 0.0
    for b in np.unique(vc[:, 0]):
        rows = np.nonzero(vc[:, 0] == b)[0]
        pts = np.nonzero(coords[:, 0] == b)[0]
        lo = vc[rows, 1:].min(0) - 1                                      # a margin of zeros on every side
        size = vc[rows, 1:].max(0) + 2 - lo + 1
        vol = torch.zeros((1, z.shape[1], int(size[2]), int(size[1]), int(size[0])), dtype=torch.float64)      # (N, C, D=z, H=y, W=x)
        ijk = vc[rows, 1:] - lo
        vol[0, :, ijk[:, 2], ijk[:, 1], ijk[:, 0]] = torch.from_numpy(z[rows]).t()
        g = (coords[pts, 1:].astype(np.float64) - lo) / (size - 1) * 2 - 1               # align_corners=True: -1 / +1 are the end voxels
        grid = torch.from_numpy(g).reshape(1, 1, 1, -1, 3)
        got = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0, 0].t().numpy()
        worst = max(worst, float(np.abs(got - y[pts]).max()))
    return worst


def test_restatement_equals_grid_sample_on_the_dense_volume():
    rng = np.random.default_rng(3)
    # multiples of 1 / 64: t is exact in fp32, so the fp32 and the float64 difference are the same number
    xyz = np.round(rng.uniform(-3.5, 3.5, size=(120, 3)) * 64) / 64
    b = np.sort(rng.integers(0, 2, size=120))
    coords = np.concatenate([b[:, None], xyz], axis=1)
    coords = np.concatenate([coords, [[0, 1.25, -2.5, 0.75], [1, 1.25, -2.5, 0.75],        # two shapes with identical xyz
                                      [1, 2.0, -1.0, 3.0]]])                               # exactly on a lattice corner
    coords = coords[np.argsort(coords[:, 0], kind="stable")].astype(np.float32)
    q = R.quantise(coords, np.zeros((coords.shape[0], 1)))
    keep = rng.uniform(size=q["voxel_coords"].shape[0]) < 0.6                              # a sparse set: points whose home is gone
    keep[q["home"][-1]] = True
    vc = q["voxel_coords"][keep]
    assert (vc[:, 1:] < 0).any() and not keep.all()
    z = rng.normal(size=(vc.shape[0], 3))
    assert np.array_equal(R.interpolate(coords, vc, z)[0], R.interpolate(coords, vc, z, exact_t=True)[0])
    assert _dense_check(coords, vc, z) <= 1e-12


def test_full_block_weights_sum_to_one_and_a_linear_map_is_reproduced():
    rng = np.random.default_rng(4)
    vc = np.array([[0, x, y, z] for z in (-1, 0) for y in (3, 4) for x in (-2, -1)])
    xyz = (np.round(rng.uniform(0, 1, size=(50, 3)) * 256) / 256 + [-2, 3, -1]).astype(np.float32)
    coords = np.concatenate([np.zeros((50, 1), dtype=np.float32), xyz], axis=1)
    ones, scale = R.interpolate(coords, vc, np.ones((8, 1)))
    assert np.abs(ones - 1).max() <= 1e-15 and np.abs(scale - 1).max() <= 1e-15
    lin = vc[:, 1:] @ np.array([[0.5], [-2.0], [3.0]]) + 0.25
    got, _ = R.interpolate(coords, vc, lin)
    assert np.abs(got - (xyz.astype(np.float64) @ np.array([[0.5], [-2.0], [3.0]]) + 0.25)).max() <= 1e-12


def test_adjoint_identity():
    rng = np.random.default_rng(6)
    coords = R.random_points(200, seed=6)
    vc = R.quantise(coords, np.zeros((200, 1)))["voxel_coords"]
    z, g = rng.normal(size=(vc.shape[0], 5)), rng.normal(size=(200, 5))
    y, _ = R.interpolate(coords, vc, z)
    dz, _, n_v = R.adjoint(coords, vc, g)
    assert abs((y * g).sum() - (z * dz).sum()) <= 1e-12 * max(1.0, abs((y * g).sum()))
    assert n_v.sum() == (R._corner_rows(R._home(coords)[1], vc) >= 0).sum() and n_v.min() >= 1


@pytest.mark.parametrize("name", ["random", "full_block", "shared_xyz", "heavy_voxel", "range_edge"])
def test_point_field_on_cpu_tensors_equals_the_restatement(name):
    from csn_amd import PointField, build_kernel_map
    coords = R.random_points(257, seed=1) if name == "random" else R.special_sets()[name].astype(np.float32)
    rng = np.random.default_rng(8)
    feats = rng.normal(size=(coords.shape[0], 3)).astype(np.float32)
    q = R.quantise(coords, feats)
    for mode in ("random_subsample", "unweighted_average"):
        f = PointField(torch.from_numpy(coords), torch.from_numpy(feats), mode)
        assert f.voxel_coords.dtype == torch.int64 and np.array_equal(f.voxel_coords.numpy(), q["voxel_coords"])
        for attr in ("home", "vox_ptr", "vox_pts"):
            t = getattr(f, attr)
            assert t.dtype == torch.int32 and np.array_equal(t.numpy(), q[attr]), attr
        b = coords[:, 0].astype(np.int64)
        assert f.offsets.tolist() == [0] + np.cumsum(np.bincount(b)).tolist()
        assert f.voxel_offsets.tolist() == [0] + np.cumsum(np.bincount(q["voxel_coords"][:, 0])).tolist()
        where, vf = f.sparse()
        assert where is f.voxel_coords and vf.dtype == torch.float32
        if mode == "random_subsample":
            assert np.array_equal(vf.numpy(), q["first"].astype(np.float32))
        else:
            bound = (q["counts"][:, None] + 2) * 2.0 ** -24 * q["mean_abs"] + 1e-30
            assert (np.abs(vf.numpy().astype(np.float64) - q["mean"]) <= bound).all()
    # the corner rows the kernels read are those of the kernel-3 map: row(v + c) = fwd[13 + cx + 3 cy + 9 cz][v]
    table = build_kernel_map(f.voxel_coords, 3).fwd.numpy()
    rows = R._corner_rows(R._home(coords)[1], q["voxel_coords"])
    for k, (cx, cy, cz) in enumerate(R.CORNERS):
        assert np.array_equal(table[13 + cx + 3 * cy + 9 * cz][q["home"]], rows[:, k])
        back = table[13 - cx - 3 * cy - 9 * cz]
        ok = back >= 0
        assert np.array_equal(q["voxel_coords"][back[ok]][:, 1:] + [cx, cy, cz], q["voxel_coords"][ok][:, 1:])
    assert f.corner_table() is f.corner_table() and np.array_equal(f.corner_table().numpy(), table)


def test_floor_of_negatives_and_the_lowest_numbered_point():
    from csn_amd import PointField
    coords = torch.tensor([[0, -0.3, -1.0, -1.5], [0, 0.3, 0.0, 1.5], [0, -0.9, -0.5, -1.01]])
    f = PointField(coords, torch.tensor([[1.0], [2.0], [3.0]]))
    assert f.voxel_coords.tolist() == [[0, -1, -1, -2], [0, 0, 0, 1]]
    assert f.home.tolist() == [0, 1, 0] and f.vox_pts.tolist() == [0, 2, 1] and f.vox_ptr.tolist() == [0, 2, 3]
    assert f.sparse()[1].tolist() == [[1.0], [2.0]]
    assert PointField(coords, torch.tensor([[1.0], [2.0], [4.0]]), "unweighted_average").sparse()[1].tolist() == [[2.5], [2.0]]


def test_bad_points_raise_value_error():
    from csn_amd import PointField
    ok = torch.tensor([[0, 0.5, 0.5, 0.5], [1, 0.5, 0.5, 0.5]])
    feats = torch.zeros(2, 3)
    PointField(ok, feats)

    def bad(r, c, v):
        t = ok.clone()
        t[r, c] = v
        return t
    cases = {"unsorted batch indices": torch.tensor([[1, 0.5, 0.5, 0.5], [0, 0.5, 0.5, 0.5]]), "non-integral b": bad(1, 0, 0.5),
             "NaN": bad(0, 2, float("nan")), "inf": bad(0, 3, float("inf")), "above the packed range": bad(1, 1, 32768.0),
             "below the packed range": bad(1, 3, -32768.5), "negative b": bad(0, 0, -1.0)}
    for what, c in cases.items():
        with pytest.raises(ValueError):
            PointField(c, feats)
            pytest.fail(what)
    with pytest.raises(ValueError):
        PointField(ok.double(), feats)
    with pytest.raises(ValueError):
        PointField(ok, torch.zeros(3, 3))
    with pytest.raises(ValueError):
        PointField(ok, feats, "weighted_average")
    with pytest.raises(ValueError):                                         # a wrong z height, before anything else is looked at
        PointField(ok, feats).interpolate(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        PointField(ok, feats).interpolate(torch.zeros(2, 1025))


def test_interpolate_refuses_cpu_tensors():
    from csn_amd import CsnError, PointField
    f = PointField(torch.tensor([[0, 0.5, 0.5, 0.5]]), torch.zeros(1, 3))
    with pytest.raises(CsnError):
        f.interpolate(torch.zeros(1, 4))


def test_sparse_is_accepted_by_build_pyramid_and_the_pyramid_is_kept():
    from csn_amd import PointField, build_pyramid
    coords = torch.from_numpy(R.random_points(300, seed=2))
    f = PointField(coords, torch.zeros(300, 3))
    where, vf = f.sparse()
    pyr = build_pyramid(where, 2)
    assert pyr.coords[0].shape[0] == vf.shape[0] == f.n_voxels
    own = f.pyramid(2)
    assert f.pyramid(2) is own and f.sparse()[0] is own and f.corner_table() is own.s1[0].fwd
    assert torch.equal(own.s1[0].fwd, pyr.s1[0].fwd) and torch.equal(own.coords[1], pyr.coords[1])
    g = f.to("cpu")
    assert torch.equal(g.home, f.home) and g.sparse()[0].n_levels == 2 and g.offsets.tolist() == f.offsets.tolist()


def test_batch_points_divides_in_float64_and_prepends_the_batch_column():
    from csn_amd import PointField, batch_points
    a = torch.tensor([[0.1, 0.2, -0.3], [0.68, 0.68, 0.68]], dtype=torch.float64)
    b = torch.tensor([[0.05, -0.05, 0.0]], dtype=torch.float64)
    coords, feats, labels = batch_points([(a, torch.ones(2, 3), torch.tensor([1, 2])), (b, torch.zeros(1, 3), torch.tensor([3]))], 0.05)
    assert coords.dtype == torch.float32 and coords[:, 0].tolist() == [0, 0, 1] and labels.tolist() == [1, 2, 3]
    assert torch.equal(coords[:2, 1:], (a / 0.05).float()) and feats.shape == (3, 3)
    assert PointField(coords, feats).voxel_coords.tolist() == [[0, 2, 4, -6], [0, 13, 13, 13], [1, 1, -1, 0]]
    assert len(batch_points([(a, torch.ones(2, 3))], 0.05)) == 2


def test_raw_entry_points_validate_on_the_host():
    """NULL pointers and bad sizes are refused before any launch (compare test_argument_validation_happens_on_the_host), so no
    GPU is needed: the non-NULL pointers below are host buffers that are never dereferenced."""
    import ctypes
    import csn_amd
    csn_amd.build()
    L = csn_amd.lib()
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ARG, PTR, DIM = -1, -3, -5
    fwd = lambda z=p, ld_z=8, nv=2, co=p, home=p, tab=p, n=3, c=8, y=p, ld_y=8: L.csn_point_interp_fwd_f32(z, ld_z, nv, co, home, tab, n, c, y, ld_y, None)
    bwd = lambda dy=p, ld=8, n=3, co=p, ptr=p, pts=p, tab=p, nv=2, c=8, dz=p, ld_dz=8: L.csn_point_interp_bwd_f32(dy, ld, n, co, ptr, pts, tab, nv, c, dz, ld_dz, None)
    mean = lambda f=p, ld=8, n=3, ptr=p, pts=p, nv=2, c=8, out=p, ld_o=8: L.csn_voxel_mean_f32(f, ld, n, ptr, pts, nv, c, out, ld_o, None)
    for name in ("z", "co", "home", "tab", "y"):
        assert fwd(**{name: None}) == ARG, name
    for name in ("dy", "co", "ptr", "pts", "tab", "dz"):
        assert bwd(**{name: None}) == ARG, name
    for name in ("f", "ptr", "pts", "out"):
        assert mean(**{name: None}) == ARG, name
    for fn in (fwd, bwd, mean):
        assert fn(n=0) == ARG and fn(nv=0) == ARG and fn(n=-5) == ARG
        assert fn(c=0) == DIM
    assert fwd(c=1025, ld_z=2048, ld_y=2048) == DIM and bwd(c=1025, ld=2048, ld_dz=2048) == DIM and mean(c=65, ld=128, ld_o=128) == DIM
    assert fwd(ld_z=7) == ARG and fwd(ld_y=7) == ARG and bwd(ld=7) == ARG and bwd(ld_dz=7) == ARG and mean(ld=7) == ARG and mean(ld_o=7) == ARG
    assert mean(n=2, nv=3) == ARG                                           # more voxels than points
    assert fwd(co=p + 4) == PTR and bwd(co=p + 8) == PTR and fwd(z=p + 2) == PTR and mean(pts=p + 1) == PTR
