"""Resident point collections on the MI355X (csn_amd.minkowski_points, include/csn_hip.h section 18) against the numpy float64
statement of tests/points_ref.py.  What is held:

  batch          coords, feats, keys, labels BIT-equal to statement (b) (the same operations in the same order, each rounded once)
  identity       equal to ``batch_points`` (as numbers: a -0.0 input may come out +0.0, 1 x + 0 z)
  normalisation  within 1 fp32 ulp of the float64 statement (the sum runs in another order than numpy's), two calls bit-equal
  from_keys      ``torch.equal`` to the constructor on every attribute
  bad input      flagged, never dereferenced: canary rows behind every output stay intact

One collection serves every test: ragged shapes of 1, 63, 64, 65, 257 and 1031 points (the wave and work-group edges of the strided
loops), one of 10 000 (the real size), one of identical points, one on a lattice of eighths (exact voxel boundaries, -0.0)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import points_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 1031, 10000]
IDENT, LATTICE = 7, 8                           # shape numbers behind the ragged ones
SIGMA, CLIP = 0.01, 0.05
CANARY_F, CANARY_I = -777.25, -7777


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _shapes():
    shapes = R.random_shapes(len(SIZES), SIZES, seed=21)
    shapes.append(np.tile(np.array([[0.25, -0.5, 0.125]], dtype=np.float32), (130, 1)))          # dyadic: its sums are exact
    k = np.arange(-4, 5, dtype=np.float32) / 8
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    lattice[lattice == 0] = np.where(np.arange((lattice == 0).sum()) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    tiny = np.array([[-2.0 ** -149, 2.0 ** -149, -2.0 ** -140]], dtype=np.float32)              # scaled down, these leave fp32: -0.0
    shapes.append(np.ascontiguousarray(np.concatenate([lattice, tiny])))
    labels = [(np.arange(s.shape[0]) * 7 + i) % 11 for i, s in enumerate(shapes)]
    return shapes, labels


@functools.lru_cache(maxsize=None)
def _collection():
    from csn_amd import PointCollection
    shapes, labels = _shapes()
    return PointCollection(list(shapes), list(labels))


def _params(n, seed, all_on=True):
    from csn_amd import AugmentSpec
    return AugmentSpec(rotate=all_on, shift_on=all_on, jitter_on=all_on, scale_on=all_on).draw(n, np.random.default_rng(seed))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_batch_is(batch, ref):
    got = {"coords": batch.coords, "feats": batch.feats, "keys": batch.keys, "labels": batch.labels}
    for name, t in got.items():
        if ref[name] is None:
            assert t is None
            continue
        a = t.cpu().numpy()
        assert a.dtype == ref[name].dtype and a.shape == ref[name].shape, name
        assert np.array_equal(a, ref[name]), (name, int((a != ref[name]).sum()))
        assert np.array_equal(_bits(a), _bits(ref[name])), name + " (bits)"
    assert batch.offsets.dtype == torch.int64 and not batch.offsets.is_cuda and np.array_equal(batch.offsets.numpy(), ref["offsets"])


# the batch of the bit statement: shape 3 twice with different numbers, out of order, every shape of the collection but the lattice
INDICES = [6, 3, 0, 5, 3, IDENT, 1, 2, 4]


@functools.lru_cache(maxsize=None)
def _main_case():
    p = _params(len(INDICES), seed=31)
    # the clip: active with either sign on some items, inactive on others (sigma diag ~ 0.02: |shift_z| 50 -> 1 >> clip)
    p.shift_z[0] = [50.0, -50.0, 0.3]
    p.shift_z[1] = [-80.0, 0.1, 60.0]
    p.shift_z[2] = [90.0, -90.0, 90.0]                                  # the 1-point shape: diagonal 0, the shift is exactly 0
    p.shift_z[5] = [-70.0, 70.0, -70.0]                                 # identical points: the same
    p.shift_z[3] = [0.2, -0.4, 0.1]
    return p


def test_batch_is_bit_equal_to_the_statement():
    shapes, labels = _shapes()
    p = _main_case()
    ref = R.project_batch(shapes, labels, INDICES, p, SIGMA, CLIP, 0.05)
    # the case reaches what it claims to reach
    t = []
    for i, s in enumerate(INDICES):
        _, e = R.bounds_item(shapes[s], p.angle[i])
        t.append((SIGMA * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) * p.shift_z[i])
    t = np.array(t)
    assert (t > CLIP).any() and (t < -CLIP).any() and ((np.abs(t) < CLIP) & (t != 0)).any()
    assert not t[2].any() and not t[5].any()
    assert (ref["coords"][:, 1:] < 0).any() and len(set(INDICES)) < len(INDICES)
    batch = _collection().batch(INDICES, p, voxel_size=0.05, shift=(SIGMA, CLIP))
    _assert_batch_is(batch, ref)
    assert int(batch.status.item()) == 0
    # degenerate shapes: the shift is exactly 0, so item 2 (one point) is ((r + 0) + jitter) scale
    q1, _ = R.project_item(shapes[0], p.angle[2], [0, 0, 0], p.jitter[2], p.scale[2], SIGMA, CLIP, 0.05)
    lo = int(batch.offsets[2])
    assert np.array_equal(batch.feats[lo:lo + 1].cpu().numpy(), q1.astype(np.float32))
    # two calls give the same bits
    again = _collection().batch(INDICES, p, voxel_size=0.05, shift=(SIGMA, CLIP))
    assert torch.equal(again.coords, batch.coords) and torch.equal(again.feats, batch.feats) and torch.equal(again.keys, batch.keys)


def test_exact_voxel_boundaries_negative_floors_and_minus_zero():
    """Scale 2 and voxel size 0.25 put every lattice point (eighths) on an exact voxel boundary, half of them below zero: floor, not
    truncation.  A jittered item sits strictly inside voxels on either side of zero.  -0.0: an item whose shift and jitter are -0.0
    keeps the sign of a -0.0 coordinate, and an item scaled by 2^-12 takes a tiny negative coordinate below fp32's range — the
    stored coordinate is -0.0 and the key is the floor of the STORED value (voxel 0), as PointField(coords, feats) has it."""
    from csn_amd import AugmentParams, PointField
    shapes, labels = _shapes()
    n = shapes[LATTICE].shape[0]
    p = AugmentParams.identity(4)
    p.scale[:] = [2.0, 2.0, 1.0, 2.0 ** -12]
    p.jitter[1] = [-0.0625, 0.03125, -0.015625]
    p.shift_z[2], p.jitter[2] = -0.0, -0.0
    idx = [LATTICE] * 4
    ref = R.project_batch(shapes, labels, idx, p, SIGMA, CLIP, 0.25)
    v = ref["coords"][:n - 1, 1:]
    assert (v == np.rint(v)).all() and (v < 0).any()
    inside = ref["coords"][n:2 * n, 1:]
    assert (np.floor(inside) != np.trunc(inside)).any()
    kept = ref["coords"][2 * n:3 * n, 1:]
    assert (np.signbit(kept) & (kept == 0)).any()
    last = ref["coords"][4 * n - 1, 1:]
    assert np.signbit(last[0]) and last[0] == 0 and last[2] == 0 and np.signbit(last[2])
    assert ref["keys"][4 * n - 1] == R.pack(3, np.zeros((1, 3)))[0]
    batch = _collection().batch(idx, p, voxel_size=0.25)
    _assert_batch_is(batch, ref)
    assert int(batch.status.item()) == 0
    field, ctor = batch.field(), PointField(batch.coords, batch.feats)
    assert torch.equal(field.home, ctor.home) and torch.equal(field.voxel_coords, ctor.voxel_coords)


def test_identity_parameters_reproduce_batch_points():
    from csn_amd import batch_points
    shapes, labels = _shapes()
    idx = [5, 0, LATTICE, 6, 1, IDENT, 2, 3, 4]
    coords, feats, target = batch_points([(torch.from_numpy(shapes[s]),) * 2 + (torch.from_numpy(labels[s]),) for s in idx], 0.05)
    batch = _collection().batch(idx, voxel_size=0.05)
    assert torch.equal(batch.coords.cpu(), coords) and torch.equal(batch.feats.cpu(), feats) and torch.equal(batch.labels.cpu(), target)
    assert batch.offsets.tolist() == np.concatenate([[0], np.cumsum([shapes[s].shape[0] for s in idx])]).tolist()
    no_labels = type(_collection())([shapes[1], shapes[0]])
    b2 = no_labels.batch([1, 0, 1], voxel_size=0.1)
    assert b2.labels is None and b2.n_points == 65 and b2.n_shapes == 3 and b2.offsets.tolist() == [0, 1, 64, 65]


FIELD_ATTRS = ("coords", "feats", "voxel_coords", "home", "vox_ptr", "vox_pts", "offsets", "voxel_offsets")


@pytest.mark.parametrize("case", ["augmented", "heavy_voxel"])
def test_from_keys_equals_the_constructor(case):
    """Every attribute ``torch.equal`` (and of one dtype), ``voxel_feats`` in both quantisation modes; heavy_voxel: a voxel size of
    0.5 puts thousands of points into one voxel."""
    from csn_amd import PointField
    vs = 0.05 if case == "augmented" else 0.5
    batch = _collection().batch(INDICES, _main_case(), voxel_size=vs, shift=(SIGMA, CLIP))
    for mode in ("random_subsample", "unweighted_average"):
        ours, theirs = batch.field(mode), PointField(batch.coords, batch.feats, mode)
        for name in FIELD_ATTRS:
            a, b = getattr(ours, name), getattr(theirs, name)
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), (name, mode)
        assert torch.equal(ours.voxel_feats, theirs.voxel_feats), mode
        assert ours.quantization_mode == mode and ours.n_voxels == theirs.n_voxels
    counts = (theirs.vox_ptr[1:] - theirs.vox_ptr[:-1])
    if case == "heavy_voxel":
        assert int(counts.max()) > 2000
    else:
        assert int(counts.max()) < 200 and theirs.n_voxels > 3000
    z = torch.randn(ours.n_voxels, 5, device="cuda")
    assert torch.equal(ours.interpolate(z), theirs.interpolate(z))         # the field works: corner table and all


def test_a_step_is_three_library_calls_and_one_host_read(L, monkeypatch):
    calls, reads = [], []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append(self.numel()) if self.is_cuda else None, real(self))[1])
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    try:
        batch = _collection().batch([3, 4], voxel_size=0.05)
        field = batch.field()
    finally:
        L.set_call_hook(None)
        monkeypatch.undo()
    assert calls == ["csn_points_bounds_f64", "csn_points_batch_f32", "csn_field_index_i32"]
    assert reads == [2 + 2]                                                 # the status word, the voxel count, B voxel-row starts
    assert field.voxel_offsets.tolist()[0] == 0 and field.voxel_offsets.tolist()[-1] == field.n_voxels


def test_neighbor_batches_are_batches_of_the_ith_neighbours():
    col = _collection()
    neighbors = [(0, [3, 1, 2]), (5, [4, 3, 0]), (2, [IDENT, 5, 6])]
    K, B = 2, 3
    p = _params(K * B, seed=41)
    out = col.neighbor_batches(neighbors, K, p, voxel_size=0.05)
    assert len(out) == K
    for i in range(K):
        ref = col.batch([n[1][i] for n in neighbors], p.slice(i * B, (i + 1) * B), voxel_size=0.05)
        for name in ("coords", "feats", "keys", "labels"):
            assert torch.equal(getattr(out[i], name), getattr(ref, name)), (i, name)
        assert torch.equal(out[i].offsets, ref.offsets)
    plain = col.neighbor_batches(neighbors, 3)
    assert len(plain) == 3 and torch.equal(plain[2].coords, col.batch([2, 0, 6]).coords)


def test_a_flagged_batch_raises_in_field():
    from csn_amd import AugmentParams
    col = _collection()
    p = AugmentParams.identity(2)
    p.scale[1] = 1.0e5                                                      # 0.9 * 1e5 / 0.05 >> 2^15
    batch = col.batch([1, 2], p, voxel_size=0.05)
    assert int(batch.status.item()) == 2
    assert (batch.keys[:63] >= 0).all() and (batch.keys[63:] == -1).any()
    with pytest.raises(ValueError, match="floor"):
        batch.field()
    for name, where in (("jitter", (0, 1)), ("shift_z", (1, 2)), ("angle", 1), ("scale", 0)):
        p = AugmentParams.identity(2)
        getattr(p, name)[where] = np.nan
        batch = col.batch([1, 2], p, voxel_size=0.05)
        assert int(batch.status.item()) == 16, name
        with pytest.raises(ValueError, match="NaN|status 16"):
            batch.field()
    p = AugmentParams.identity(2)
    p.shift_z[0, 0] = np.inf                                                # clipped to a finite shift, still refused
    batch = col.batch([1, 2], p, voxel_size=0.05)
    assert int(batch.status.item()) == 16 and bool(torch.isfinite(batch.coords).all())
    with pytest.raises(ValueError, match="status 16"):
        batch.field()


def _raw_batch(L, col, idx, out_off, n_out, params=None, offsets=None, n_shapes=None, n_total=None, rows=None, max_points=1031):
    """The two raw launches on buffers with ``pad`` canary rows behind their last row; returns the buffers and the status word."""
    pad = 64
    n = len(idx)
    rows = n_out if rows is None else rows
    dev = col.device
    items = torch.tensor([idx, out_off], dtype=torch.int64, device=dev)
    par = torch.from_numpy(np.tile([1.0, 0.0, 0, 0, 0, 0, 0, 0, 1.0], (n, 1)) if params is None else params).to(dev)
    bounds = torch.full((n + pad, 6), CANARY_F, dtype=torch.float64, device=dev)
    coords = torch.full((rows + pad, 4), CANARY_F, device=dev)
    feats = torch.full((rows + pad, 3), CANARY_F, device=dev)
    keys = torch.full((rows + pad,), CANARY_I, dtype=torch.int64, device=dev)
    labels = torch.full((rows + pad,), CANARY_I, dtype=torch.int64, device=dev)
    status = torch.zeros(1 + pad, dtype=torch.int32, device=dev)
    offsets = col.offsets_dev if offsets is None else offsets
    n_shapes = col.n_shapes if n_shapes is None else n_shapes
    n_total = col.n_points if n_total is None else n_total
    st = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    L.check(lib.csn_points_bounds_f64(col.points.data_ptr(), offsets.data_ptr(), n_shapes, n_total, items[0].data_ptr(), par.data_ptr(), n,
                                      bounds.data_ptr(), status.data_ptr(), st), "csn_points_bounds_f64")
    L.check(lib.csn_points_batch_f32(col.points.data_ptr(), col.labels.data_ptr(), offsets.data_ptr(), n_shapes, n_total,
                                     items[0].data_ptr(), items[1].data_ptr(), par.data_ptr(), bounds.data_ptr(), n, max_points, SIGMA, CLIP, 0.05,
                                     coords.data_ptr(), feats.data_ptr(), labels.data_ptr(), keys.data_ptr(), n_out, status.data_ptr(), st),
            "csn_points_batch_f32")
    torch.cuda.synchronize()
    assert (bounds[n:] == CANARY_F).all() and (coords[rows:] == CANARY_F).all() and (feats[rows:] == CANARY_F).all()
    assert (keys[rows:] == CANARY_I).all() and (labels[rows:] == CANARY_I).all() and not status[1:].any()
    return {"bounds": bounds, "coords": coords, "feats": feats, "keys": keys, "labels": labels, "status": int(status[0].item())}


def test_bad_values_are_flagged_and_never_dereferenced(L):
    """Shape numbers, CSR offsets, output rows, sort positions and voxel numbers outside their arrays: the item or point is skipped,
    flag 32 is raised, and nothing behind the buffers' last row is touched."""
    col = _collection()
    # a good call first: the raw path gives what batch() gives
    good = _raw_batch(L, col, [1, 2], [0, 63], 127)
    ref = col.batch([1, 2], voxel_size=0.05)
    assert good["status"] == 0 and torch.equal(good["coords"][:127], ref.coords) and torch.equal(good["keys"][:127], ref.keys)
    assert torch.equal(good["labels"][:127], ref.labels)
    # shape numbers outside the collection: skipped, their rows keep the canary, the good item is written
    bad = _raw_batch(L, col, [-1, 1, col.n_shapes, 1 << 40], [0, 0, 63, 63], 127)
    assert bad["status"] == 32 and torch.equal(bad["coords"][:63, 1:], ref.coords[:63, 1:]) and (bad["coords"][63:127] == CANARY_F).all()
    assert not bad["bounds"][0].any() and not bad["bounds"][2].any() and not bad["bounds"][3].any()
    # output rows outside [0, n_out): a negative start, a start behind the end, an item that would run over the end
    for out_off in ([0, -5], [0, 200], [0, 70], [0, 1 << 50]):
        bad = _raw_batch(L, col, [1, 2], out_off, 127)
        assert bad["status"] == 32 and torch.equal(bad["coords"][:63], ref.coords[:63]) and (bad["keys"][63:127] == CANARY_I).all(), out_off
    # a CSR that descends or leaves the point array
    off = torch.tensor([0, 5, 3, 4000, 1 << 45], dtype=torch.int64, device="cuda")
    bad = _raw_batch(L, col, [0, 1, 2, 3], [0, 5, 10, 15], 20, offsets=off, n_shapes=4, n_total=1000)
    assert bad["status"] == 32 and (bad["coords"][5:20] == CANARY_F).all() and (bad["coords"][:5, 0] == 0).all()
    # more than 2^15 items (of the one-point shape): flag 1 from item 2^15 on, every row still written inside its buffer
    n = (1 << 15) + 3
    many = _raw_batch(L, col, [0] * n, list(range(n)), n, max_points=1)
    assert many["status"] == 1 and (many["keys"][:1 << 15] >= 0).all() and (many["keys"][1 << 15:n] == -1).all()
    assert (many["coords"][:n, 0] == torch.arange(n, device="cuda")).all()
    # the normalisation skips what the batch kernels skip
    pts = col.points[:1000].clone()
    out = torch.full((1000 + 64, 3), CANARY_F, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.lib().csn_points_normalize_f32(pts.data_ptr(), off.data_ptr(), 4, 1000, 0, out.data_ptr(), status.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "csn_points_normalize_f32")
    assert int(status.item()) == 32 and (out[5:] == CANARY_F).all() and bool(torch.isfinite(out[:5]).all())


def test_field_index_flags_positions_and_voxel_numbers_outside_their_arrays(L):
    n, n_vox, pad = 300, 40, 32
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(0, n_vox, (n,), generator=g)
    keys[:n_vox] = torch.arange(n_vox)
    keys = keys.cuda()
    skeys, order = torch.sort(keys, stable=True)
    vid = torch.cat([skeys.new_zeros(1), (skeys[1:] != skeys[:-1]).cumsum(0)])

    def run(order, vid):
        home = torch.full((n + pad,), CANARY_I, dtype=torch.int32, device="cuda")
        vox_ptr = torch.full((n_vox + 1 + pad,), CANARY_I, dtype=torch.int32, device="cuda")
        vox_pts = torch.full((n + pad,), CANARY_I, dtype=torch.int32, device="cuda")
        uniq = torch.full((n_vox + pad,), CANARY_I, dtype=torch.int64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(L.lib().csn_field_index_i32(skeys.data_ptr(), order.data_ptr(), vid.data_ptr(), n, n_vox, home.data_ptr(), vox_ptr.data_ptr(),
                                            vox_pts.data_ptr(), uniq.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "csn_field_index_i32")
        torch.cuda.synchronize()
        assert (home[n:] == CANARY_I).all() and (vox_ptr[n_vox + 1:] == CANARY_I).all() and (vox_pts[n:] == CANARY_I).all()
        assert (uniq[n_vox:] == CANARY_I).all()
        return home[:n], vox_ptr[:n_vox + 1], vox_pts[:n], uniq[:n_vox], int(status.item())

    home, vox_ptr, vox_pts, uniq, word = run(order, vid)
    counts = torch.bincount(keys, minlength=n_vox)
    assert word == 0 and torch.equal(home.long(), keys) and torch.equal(uniq, torch.arange(n_vox, device="cuda"))
    assert torch.equal(vox_ptr.long(), torch.cat([counts.new_zeros(1), counts.cumsum(0)])) and torch.equal(vox_pts.long(), order)
    bad_order, bad_vid = order.clone(), vid.clone()
    bad_order[[0, 7, 299]] = torch.tensor([-1, n, 1 << 40], device="cuda")
    bad_vid[[3, 150, 298]] = torch.tensor([-2, n_vox, 1 << 35], device="cuda")
    home, vox_ptr, vox_pts, uniq, word = run(bad_order, bad_vid)
    assert word == 32 and (vox_pts[[0, 7, 299]] == -1).all() and int(vox_ptr[n_vox]) == n


def test_raw_entry_points_reject_bad_arguments_on_the_host(L):
    R.abi_rejections(L.lib())


@pytest.mark.parametrize("method", ["sphere", "box"])
def test_normalisation(L, method):
    from csn_amd import PointCollection
    shapes, _ = _shapes()
    # (without the lattice: its centre point sits on the centroid up to rounding, where the quotient is all cancellation noise)
    raw = [(s * np.float32(1.7) + np.array([0.4, -0.2, 0.1], dtype=np.float32) * (i % 3)).astype(np.float32)
           for i, s in enumerate(shapes[:LATTICE])]
    raw[IDENT] = shapes[IDENT]                                              # (kept dyadic: its centroid is exact in any order)
    col = PointCollection(raw)
    before = col.points.clone()
    assert col.normalize(method) is col and col.normalized == method
    got = col.points.cpu().numpy()
    off = col.offsets.tolist()
    worst = 0
    for s, xyz in enumerate(raw):
        ref = R.normalize64(xyz, method).astype(np.float32)
        d = R.ulp32_distance(got[off[s]:off[s + 1]], ref)
        worst = max(worst, int(d.max()))
        assert d.max() <= 1, (s, int(d.max()))
    print(f"[points] normalize({method}) vs float64: worst {worst} fp32 ulp")
    # the clamp: one point, and identical points, sit on their centroid: radius 0 -> 2 eps_fp32, outputs exactly 0
    assert not got[off[0]:off[1]].any() and not got[off[IDENT]:off[IDENT + 1]].any()
    if method == "sphere":
        norms = np.linalg.norm(got[off[6]:off[7]].astype(np.float64), axis=1)
        assert abs(norms.max() - 1.0) < 1e-6
    # a second call on a fresh copy gives the same bits; out of place equals in place
    again = PointCollection(raw).normalize(method)
    assert torch.equal(again.points, col.points)
    out = torch.full_like(before, CANARY_F)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.lib().csn_points_normalize_f32(before.data_ptr(), col.offsets_dev.data_ptr(), col.n_shapes, col.n_points,
                                             ("sphere", "box").index(method), out.data_ptr(), status.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "csn_points_normalize_f32")
    assert int(status.item()) == 0 and torch.equal(out, col.points)


def test_end_to_end_equals_the_host_path():
    """HRNetSimCSN2S on 2 shapes of ~300 points: the collection's batch and field against batch_points + PointField(...) on the same
    points — identical tensors into identical launches, so logits, loss and a weight gradient are ``torch.equal``."""
    from csn_amd import HRNetSimCSN2S, PointCollection, PointField, batch_points, seg_loss
    torch.manual_seed(5)
    shapes = R.random_shapes(2, [300, 293], seed=9)
    shapes = [(s * np.float32(0.3)).astype(np.float32) for s in shapes]
    labels = [np.random.default_rng(i).integers(0, 6, size=s.shape[0]) for i, s in enumerate(shapes)]
    model = HRNetSimCSN2S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().train()

    def run(field, target):
        m = copy.deepcopy(model)                                            # the same weights and buffers for either path ...
        torch.manual_seed(23)                                               # ... and the same seeds: the attention draws its from torch's generator
        field.pyramid(2)
        plog = field.interpolate(m(field.sparse()))
        loss, _ = seg_loss(plog, target, field.offsets)
        loss.backward()
        weight = next(p for p in m.parameters() if p.dim() > 1)
        return plog.detach(), loss.detach(), weight.grad

    batch = PointCollection(shapes, labels).batch([0, 1], voxel_size=0.05)
    a = run(batch.field(), batch.labels)
    coords, feats, target = batch_points([(torch.from_numpy(s), torch.from_numpy(s), torch.from_numpy(l)) for s, l in zip(shapes, labels)], 0.05)
    b = run(PointField(coords.cuda(), feats.cuda()), target.cuda())
    assert a[0].shape == (593, 6) and bool(torch.isfinite(a[1])) and float(a[2].abs().max()) > 0
    for x, y, name in zip(a, b, ("logits", "loss", "weight gradient")):
        assert torch.equal(x, y), name
