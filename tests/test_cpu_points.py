"""CPU-side checks (no GPU needed) of csn_amd.minkowski_points: this project's statement of the augmentation chain against the
reference's order of operations (both in tests/points_ref.py), the reference's fp32 normalisation against the float64 statement, the
drawn numbers, the argument errors and the raw entry points' host-side rejections."""
import numpy as np
import pytest
import torch

from tests import points_ref as R

U = 2.0 ** -24


@pytest.fixture(scope="module")
def shapes():
    return R.random_shapes(40, 10000, seed=7)


def test_project_order_matches_reference_order(shapes):
    """(b) vs (a), PartNet bounds, rotation + shift + jitter + scale on, voxel size 0.05: the fp32 outputs within 1 fp32 ulp; the home
    voxel equal wherever the float64 voxel coordinate is farther than 1e-6 from an integer, and that exclusion is <= 1 % of the
    points."""
    from csn_amd import AugmentSpec
    spec = AugmentSpec(rotate=True, shift_on=True, jitter_on=True, scale_on=True)
    p = spec.draw(len(shapes), np.random.default_rng(11))
    sigma, clip = spec.shift
    worst = differing = excluded = homes = 0
    for i, xyz in enumerate(shapes):
        args = (xyz, p.angle[i], p.shift_z[i], p.jitter[i], p.scale[i], sigma, clip, 0.05)
        qa, va = R.reference_item(*args)
        qb, vb = R.project_item(*args)
        for a, b in ((qa, qb), (va, vb)):
            d = R.ulp32_distance(a.astype(np.float32), b.astype(np.float32))
            worst, differing = max(worst, int(d.max())), differing + int((d > 0).sum())
        near = (np.abs(vb - np.rint(vb)) <= 1e-6).any(axis=1)
        same = (np.floor(va.astype(np.float32)) == np.floor(vb.astype(np.float32))).all(axis=1)
        excluded, homes = excluded + int(near.sum()), homes + int((~same).sum())
        assert same[~near].all()
    n = sum(s.shape[0] for s in shapes)
    print(f"[points] (b) vs (a): worst {worst} ulp, {differing} of {6 * n} fp32 values differ, {homes} of {n} home voxels differ, "
          f"{excluded} points within 1e-6 of a voxel boundary")
    assert worst <= 1
    assert excluded <= 0.01 * n


@pytest.mark.parametrize("method", ["sphere", "box"])
def test_reference_fp32_normalisation_is_near_the_float64_statement(method):
    """The reference normalises in fp32 with a running mean over n points; its distance from the float64 statement is bounded by
    (n + 8) 2^-24 max|p| / r: n - 1 adds and a division for the mean, one subtraction, three roundings for the radius, the final
    division and the fp32 rounding of the statement itself.  A statement about the reference's rounding, not a tolerance of ours."""
    worst = 0.0
    for s, xyz in enumerate(R.random_shapes(6, [10000, 1031, 257, 65, 10000, 3000], seed=3)):
        xyz = (xyz + np.float32(0.25 * s)).astype(np.float32)                     # an off-centre shape: the mean matters
        ref = R.normalize_reference(xyz, method)
        assert ref.dtype == np.float32
        out = R.normalize64(xyz, method)
        d = xyz.astype(np.float64) - xyz.astype(np.float64).sum(axis=0) / xyz.shape[0]
        r = np.abs(d[0] / out[0]).max() if np.abs(out[0]).max() > 0 else 1.0
        bound = (xyz.shape[0] + 8) * U * np.abs(xyz).max() / r
        err = np.abs(ref.astype(np.float64) - out).max()
        worst = max(worst, err / U)
        assert err <= bound, (s, err, bound)
    print(f"[points] reference fp32 normalisation ({method}) vs float64: worst {worst:.1f} x 2^-24")


def test_draw_bounds_neutral_values_order_and_reproducibility():
    from csn_amd import AugmentParams, AugmentSpec
    spec = AugmentSpec(rotate=True, shift_on=True, jitter_on=True, scale_on=True, jitter_bound=(0.25, 0.1, 0.05))
    p = spec.draw(200, np.random.default_rng(5))
    assert p.angle.dtype == p.shift_z.dtype == p.jitter.dtype == p.scale.dtype == np.float64
    assert p.angle.shape == (200,) and p.shift_z.shape == (200, 3) and p.jitter.shape == (200, 3) and p.scale.shape == (200,)
    assert (p.angle >= spec.rotation_bound[0]).all() and (p.angle <= spec.rotation_bound[1]).all()
    assert (np.abs(p.jitter) <= np.array(spec.jitter_bound)).all() and np.abs(p.jitter[:, 0]).max() > 0.1
    assert (p.scale >= 0.75).all() and (p.scale <= 1.25).all() and p.scale.std() > 0.05
    assert abs(p.shift_z.mean()) < 0.2 and 0.8 < p.shift_z.std() < 1.2
    # the same generator state gives the same numbers
    q = spec.draw(200, np.random.default_rng(5))
    for name in ("angle", "shift_z", "jitter", "scale"):
        assert np.array_equal(getattr(p, name), getattr(q, name))
    # per item: angle, three shift normals, jitter x, y, z, scale — the reference's order
    rng = np.random.default_rng(5)
    for i in range(3):
        assert p.angle[i] == rng.uniform(*spec.rotation_bound)
        assert np.array_equal(p.shift_z[i], rng.standard_normal(3))
        for k in range(3):
            assert p.jitter[i, k] == rng.uniform(-spec.jitter_bound[k], spec.jitter_bound[k])
        assert p.scale[i] == rng.uniform(*spec.scale_bound)
    # a disabled transform draws nothing and is neutral
    only_scale = AugmentSpec(scale_on=True).draw(4, np.random.default_rng(9))
    assert not only_scale.angle.any() and not only_scale.shift_z.any() and not only_scale.jitter.any()
    rng = np.random.default_rng(9)
    assert np.array_equal(only_scale.scale, [rng.uniform(0.75, 1.25) for _ in range(4)])
    none = AugmentSpec().draw(3, np.random.default_rng(1))
    ident = AugmentParams.identity(3)
    for name in ("angle", "shift_z", "jitter", "scale"):
        assert np.array_equal(getattr(none, name), getattr(ident, name))


def test_spec_defaults_distort_partnet_and_identity():
    from csn_amd import AugmentParams, AugmentSpec
    s = AugmentSpec()
    assert s.rotation_bound == (-5 * np.pi / 180.0, 5 * np.pi / 180) and s.jitter_bound == (0.25, 0.25, 0.25)
    assert s.scale_bound == (0.75, 1.25) and s.shift == (0.01, 0.05)
    assert not (s.rotate or s.shift_on or s.jitter_on or s.scale_on)
    d = AugmentSpec.distort_partnet()
    assert d.rotate and d.jitter_on and d.scale_on and not d.shift_on
    i = AugmentParams.identity(5)
    assert len(i) == 5 and not i.angle.any() and not i.shift_z.any() and not i.jitter.any() and (i.scale == 1).all()
    packed = i.packed()
    assert packed.shape == (5, 9) and (packed[:, 0] == 1).all() and not packed[:, 1:8].any() and (packed[:, 8] == 1).all()
    with pytest.raises(ValueError):
        AugmentParams(np.zeros(2), np.zeros((3, 3)), np.zeros((2, 3)), np.ones(2))
    with pytest.raises(ValueError):
        AugmentSpec(shift=(0.01, 0.0))


def test_argument_errors_come_before_any_device_work():
    from csn_amd import AugmentParams, CsnError, PointCollection, PointField
    pts = R.random_shapes(3, [5, 7, 4], seed=1)
    labels = [np.arange(p.shape[0]) % 3 for p in pts]
    col = PointCollection(pts, labels, device="cpu")
    assert col.n_shapes == 3 and col.n_points == 16 and col.offsets.tolist() == [0, 5, 12, 16]
    assert col.points.dtype == torch.float32 and col.labels.dtype == torch.int32 and col.offsets.dtype == torch.int64
    same = PointCollection(np.stack([pts[0], pts[0]]), np.stack([labels[0], labels[0]]), device="cpu")      # the (S, P, 3) form
    assert same.offsets.tolist() == [0, 5, 10]
    for bad in ([p.astype(np.float64) for p in pts], [p[:, :2] for p in pts], [pts[0], pts[1][:0]], [], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError):
            PointCollection(bad, device="cpu")
    with pytest.raises(ValueError):
        PointCollection(pts, labels[:2], device="cpu")
    with pytest.raises(ValueError):
        PointCollection(pts, [l.astype(np.float32) for l in labels], device="cpu")
    for bad in ([3], [-1], [0, 1, 99], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            col.batch(bad)
    with pytest.raises(ValueError, match="params"):
        col.batch([0, 1], AugmentParams.identity(3))
    for vs in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            col.batch([0, 1], voxel_size=vs)
    with pytest.raises(ValueError, match="neighbours"):
        col.neighbor_batches([(0, [1, 2]), (1, [0])], K=2)
    with pytest.raises(ValueError):
        col.neighbor_batches([(0, [1, 2])], K=0)
    with pytest.raises(ValueError, match="params"):
        col.neighbor_batches([(0, [1, 2]), (1, [0, 2])], K=2, params=AugmentParams.identity(2))
    with pytest.raises(ValueError):
        col.neighbor_batches([(0, [1, 7])], K=2)
    with pytest.raises(ValueError, match="method"):
        col.normalize("cube")
    # valid arguments on a host-held collection: there is no CPU path
    with pytest.raises(CsnError):
        col.batch([0, 1])
    with pytest.raises(CsnError):
        col.normalize()
    coords, feats = torch.zeros(4, 4), torch.zeros(4, 3)
    keys, status = torch.zeros(4, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(CsnError):
        PointField.from_keys(coords, feats, keys, status, [0, 4])
    for bad in ([0, 3], [0, 2, 2, 4], [1, 4]):
        with pytest.raises(ValueError, match="offsets"):
            PointField.from_keys(coords, feats, keys, status, bad)
    with pytest.raises(ValueError):
        PointField.from_keys(coords, feats, keys.int(), status, [0, 4])
    with pytest.raises(ValueError):
        PointField.from_keys(coords, feats, keys, status, [0, 4], quantization_mode="median")


def test_from_h5_files_round_trip_or_named_import_error(tmp_path):
    from csn_amd import PointCollection
    try:
        import h5py
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            PointCollection.from_h5_files(["a.h5"], str(tmp_path))
        return
    rng = np.random.default_rng(0)
    data = [rng.standard_normal((s, 50, 3)).astype(np.float32) for s in (2, 3)]
    labs = [rng.integers(0, 5, (s, 50)).astype(np.int32) for s in (2, 3)]
    for i in range(2):
        with h5py.File(tmp_path / f"{i}.h5", "w") as f:
            f["data"], f["label_seg"] = data[i], labs[i]
    col = PointCollection.from_h5_files(["0.h5", "1.h5"], str(tmp_path), device="cpu")
    assert col.n_shapes == 5 and col.offsets.tolist() == [0, 50, 100, 150, 200, 250]
    assert np.array_equal(col.points.numpy(), np.concatenate(data).reshape(-1, 3))
    assert np.array_equal(col.labels.numpy(), np.concatenate(labs).reshape(-1))


def test_entry_points_validate_on_the_host():
    import csn_amd
    csn_amd.build()
    R.abi_rejections(csn_amd.lib())
