"""The native kernel-map backend on the MI355X (include/csn_hip.h section 17, csrc/kernel_map.hip; ``backend="hip"`` of
csn_amd.minkowski_conv.build_kernel_map and csn_amd.minkowski_hrnet.build_pyramid) against two references that are not the code
under test: the torch backend on the same device tensors (``torch.equal`` on every table and coordinate set — the results are
integers, there is no tolerance) and the dictionary restatement ``tests/sparse_conv_ref.geometry``."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777
SETS = {"single_voxel": R.single_voxel, "dense_block": R.dense_block, "two_clusters": R.two_clusters,
        **{f"n{n}": functools.partial(R.random_set, n) for n in (63, 64, 65, 257, 1031)}}


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


def _dev(rows):
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


def _shuffled(rows, seed):
    rows = [list(r) for r in rows]
    np.random.default_rng(seed).shuffle(rows)
    return rows


def _tables(g):
    """(fwd (KV, n_out), bwd (KV, n_in)) int32 of a ``sparse_conv_ref.Geometry``."""
    fwd = torch.full((g.KV, g.n_out), -1, dtype=torch.int32)
    bwd = torch.full((g.KV, g.n_in), -1, dtype=torch.int32)
    for kidx, (j, i) in enumerate(g.pairs):
        fwd[kidx, j] = i.int()
        bwd[kidx, i] = j.int()
    return fwd, bwd


def _same(a, b):
    """Two ``KernelMap`` objects are indistinguishable."""
    for name in ("in_coords", "out_coords", "fwd"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), name
    assert (a.bwd_table is None) == (b.bwd_table is None)
    if a.bwd_table is not None:
        assert a.bwd_table.dtype == b.bwd_table.dtype == torch.int32 and a.bwd_table.is_contiguous() and torch.equal(a.bwd_table, b.bwd_table)
    assert a.fwd.is_contiguous() and a.fwd.dtype == torch.int32 and a.out_coords.dtype == torch.int64
    assert (a.kernel_size, a.stride, a.in_tensor_stride, a.out_tensor_stride, a.transposed) == \
           (b.kernel_size, b.stride, b.in_tensor_stride, b.out_tensor_stride, b.transposed)


def _both(coords, g=None, **kw):
    """The map under both backends, compared; against the dictionary geometry ``g`` too where one is given."""
    from csn_amd.minkowski_conv import build_kernel_map
    hip, ref = build_kernel_map(coords, backend="hip", **kw), build_kernel_map(coords, backend="torch", **kw)
    _same(hip, ref)
    if g is not None:
        fwd, bwd = _tables(g)
        assert torch.equal(hip.fwd.cpu(), fwd) and torch.equal(hip.bwd.cpu(), bwd)
    return hip


@pytest.mark.parametrize("ts", [1, 2, 4])
@pytest.mark.parametrize("name", list(SETS))
def test_every_geometry_equals_the_torch_backend_and_the_dictionary(L, name, ts):
    rows = SETS[name](ts=ts)
    coords = _dev(rows)
    for k in (1, 3, 5):                                                     # stride 1: no second table
        m = _both(coords, R.geometry("s1", rows, k, ts)[0], kernel_size=k, stride=1, tensor_stride=ts)
        assert m.bwd_table is None and m.out_coords is m.in_coords
    g, out = R.geometry("s2", rows, 3, ts)                                  # stride 2, generated coordinates
    m = _both(coords, g, kernel_size=3, stride=2, tensor_stride=ts)
    assert m.out_coords.tolist() == [list(c) for c in out] and m.bwd_table is not None
    given = _shuffled(out, 1)                                               # stride 2 onto a given, shuffled coarse set
    _both(coords, R.Geometry([tuple(r) for r in rows], [tuple(r) for r in given], 3, ts, 1),
          kernel_size=3, stride=2, tensor_stride=ts, out_coords=_dev(given))
    fine = _shuffled(rows, 2)                                               # transposed: the searched set's rows are not in key order
    coarse = _shuffled(out, 3)
    _both(_dev(coarse), R.geometry("tr", coarse, 3, ts, fine=fine)[0], kernel_size=3, stride=2,
          tensor_stride=2 * ts, out_coords=_dev(fine), transposed=True)


def _kidx(ox, oy, oz, k=3):
    r = k // 2
    return (ox + r) + k * (oy + r) + k * k * (oz + r)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_range_edges_read_no_voxel_and_never_carry_into_the_next_field(L, axis):
    """Voxels at -32768 and 32767 on one axis with a neighbour one step inside, and the DECOYS a carry would find: the key of
    [0, x, y, 32767] plus one is the key of [0, x, y + 1, -32768] (z carries into y, y into x, x into the batch index), and minus one
    from -32768 borrows the other way."""
    lo, hi = -32768, 32767
    e = [0, 0, 0]
    e[axis] = 1
    base = [3, -5, 7]
    at = lambda v: [0] + [v if a == axis else base[a] for a in range(3)]
    up, down_ = at(hi), at(lo)
    rows = [up, at(hi - 1), down_, at(lo + 1)]
    if axis == 0:
        decoys = [[1, lo, base[1], base[2]]]                               # x + 1 carries into b (a borrow from b = 0 has no voxel)
    else:
        carry, borrow = at(lo), at(hi)
        carry[axis] += 1                                                    # column ``axis`` is the next more significant field
        borrow[axis] -= 1
        decoys = [carry, borrow]
    rows = rows + decoys
    assert len({tuple(r) for r in rows}) == len(rows)
    for k in (3, 5):
        m = _both(_dev(rows), R.geometry("s1", rows, k, 1)[0], kernel_size=k, stride=1, tensor_stride=1)
        plus, minus = _kidx(*e, k=k), _kidx(*[-v for v in e], k=k)
        assert m.fwd[plus, 0].item() == -1 and m.fwd[minus, 0].item() == 1        # the voxel at 32767: nothing above, its neighbour below
        assert m.fwd[minus, 2].item() == -1 and m.fwd[plus, 2].item() == 3        # the voxel at -32768
    # the same through the stride-2 and transposed tables (floor at the lower edge, offsets from both edges)
    m = _both(_dev(rows), R.geometry("s2", rows, 3, 1)[0], kernel_size=3, stride=2, tensor_stride=1)
    coarse = m.out_coords.tolist()
    _both(_dev(coarse), R.geometry("tr", coarse, 3, 1, fine=rows)[0], kernel_size=3, stride=2, tensor_stride=2, out_coords=_dev(rows),
          transposed=True)


def test_offsets_never_cross_batch_indices_and_the_last_batch_index_is_taken(L):
    block = [r[1:] for r in R.dense_block()]
    rows = [[0] + r for r in block] + [[1] + r for r in block]              # two shapes with identical xyz
    m = _both(_dev(rows), R.geometry("s1", rows, 3, 1)[0], kernel_size=3, stride=1, tensor_stride=1)
    b = m.in_coords[:, 0]
    hit = m.fwd >= 0
    assert bool((b[m.fwd.clamp(min=0).long()] == b[None, :])[hit].all()) and int(hit.sum()) > 27 * 8
    d = _both(_dev(rows), R.geometry("s2", rows, 3, 1)[0], kernel_size=3, stride=2, tensor_stride=1)
    hit = d.fwd >= 0
    assert bool((b[d.fwd.clamp(min=0).long()] == d.out_coords[:, 0][None, :])[hit].all())
    rows = [[32767] + r for r in block] + [[0] + r for r in block[:5]] + [[32766] + r for r in block]
    m = _both(_dev(rows), R.geometry("s1", rows, 5, 1)[0], kernel_size=5, stride=1, tensor_stride=1)
    assert int(m.out_coords[:, 0].max()) == 32767


def _raw_map(L, set_keys, set_rows, query_keys, k, step, table, status):
    L.check(L.lib().csn_kernel_map_i32(set_keys.data_ptr(), None if set_rows is None else set_rows.data_ptr(), set_keys.numel(),
                                       query_keys.data_ptr(), query_keys.numel(), k, step, table.data_ptr(), status.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "csn_kernel_map_i32")


def test_the_search_ends_inside_its_array_at_both_ends(L):
    """The set is a VIEW inside a larger key buffer whose neighbours hold exactly the keys the queries ask for: a query below the
    smallest key and one above the largest read -1, which a search that looked one element outside its array would not."""
    from csn_amd.minkowski_conv import _pack
    rows = sorted(tuple(r) for r in R.random_set(65))
    below, above = (0, -9, 0, 0), (1, 9, 0, 0)                             # outside the set's cube on either side
    assert below < rows[0] and above > rows[-1]
    buf = _pack(_dev([below] + [list(r) for r in rows] + [above]))
    assert bool((buf[1:] > buf[:-1]).all())
    view = buf[1:-1]
    queries = _pack(_dev([below, above, rows[0], rows[-1], rows[31]]))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = torch.full((1, 5), CANARY, dtype=torch.int32, device="cuda")
    _raw_map(L, view, None, queries, 1, 1, table, status)
    assert table.tolist() == [[-1, -1, 0, 64, 31]] and status.item() == 0
    # kernel 3 from the two outside points: every offset still ends inside the view (and finds nothing)
    table = torch.full((27, 2), CANARY, dtype=torch.int32, device="cuda")
    _raw_map(L, view, None, queries[:2], 3, 1, table, status)
    assert bool((table == -1).all()) and status.item() == 0
    # a set of one key
    table = torch.full((27, 5), CANARY, dtype=torch.int32, device="cuda")
    _raw_map(L, buf[1:2], None, queries, 3, 1, table, status)
    want = torch.full((27, 5), -1, dtype=torch.int32)
    want[13, 2] = 0
    want[:, 3:] = _tables(R.geometry("s1", rows, 3, 1)[0])[0][:, [64, 31]]
    want[:, 3:][want[:, 3:] != 0] = -1                                       # only row 0 of the set is there
    assert torch.equal(table.cpu(), want) and status.item() == 0


@pytest.mark.parametrize("n_query", [1, 65])
@pytest.mark.parametrize("k", [3, 5])
def test_the_table_is_written_and_nothing_around_it(L, n_query, k):
    from csn_amd.minkowski_conv import _pack, build_kernel_map
    rows = R.random_set(65)
    coords = _dev(rows)
    keys = _pack(coords)
    skeys, perm = torch.sort(keys)
    KV, pad = k ** 3, 70
    buf = torch.full((pad + KV * n_query + pad,), CANARY, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _raw_map(L, skeys, perm.int(), keys[:n_query].contiguous(), k, 1, buf[pad:pad + KV * n_query], status)
    assert bool((buf[:pad] == CANARY).all()) and bool((buf[pad + KV * n_query:] == CANARY).all()) and status.item() == 0
    want = build_kernel_map(coords, kernel_size=k, backend="torch").fwd[:, :n_query]
    assert torch.equal(buf[pad:pad + KV * n_query].view(KV, n_query), want)


def test_raw_keys_floors_and_flags(L):
    """(17a) and (17b) by themselves: the keys are ``_pack``'s, the flags are per failure kind, the coarser keys floor."""
    from csn_amd.minkowski_conv import _pack
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream

    def keys_of(rows, ts):
        c = _dev(rows)
        keys = torch.empty(c.shape[0], dtype=torch.int64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.csn_coord_keys_i64(c.data_ptr(), c.shape[0], ts, keys.data_ptr(), status.data_ptr(), st), "csn_coord_keys_i64")
        return c, keys, status.item()

    rows = R.random_set(257, ts=2) + [[32767, -32768, 32766, 0], [0, 32766, -32768, -2]]
    c, keys, flag = keys_of(rows, 2)
    assert flag == 0 and torch.equal(keys, _pack(c))
    good = [0, 4, -4, 8]
    for bad, want in (([32768, 0, 0, 0], 1), ([-1, 0, 0, 0], 1), ([0, 32768, 0, 0], 2), ([0, 0, -32772, 0], 2), ([0, 0, 0, 32768], 2),
                      ([0, 2, 0, 0], 4), ([0, 0, -3, 0], 4), ([0, 0, 0, 1], 4), ([40000, 0, 40000, 1], 7)):
        for n_before in (0, 64, 130):                                       # the flag leaves whichever wave finds it
            assert keys_of([good] * n_before + [bad] + [good] * 3, 4)[2] == want, (bad, n_before)
    assert keys_of([[0, -4, -8, 4]], 4)[2] == 0                            # negative multiples are multiples
    for ts in (2, 4, 3):
        down = torch.empty_like(keys)
        L.check(lib.csn_coord_down_i64(keys.data_ptr(), keys.numel(), ts, down.data_ptr(), st), "csn_coord_down_i64")
        want = c.clone()
        want[:, 1:] = torch.div(c[:, 1:], ts, rounding_mode="floor") * ts
        if ts == 3:                                                         # -32768 floors to -32769 at 3: outside the fields
            ok = (want[:, 1:] >= -32768).all(dim=1)
            assert int(ok.sum()) == len(rows) - 2
            assert torch.equal(down[ok], _pack(want[ok]))
        else:
            assert torch.equal(down, _pack(want))
    one = _pack(_dev([[5, -1, -2, -3]]))
    L.check(lib.csn_coord_down_i64(one.data_ptr(), 1, 2, one.data_ptr(), st), "csn_coord_down_i64")        # in place
    assert torch.equal(one, _pack(_dev([[5, -2, -2, -4]])))


def test_bad_coordinates_raise_the_torch_backends_messages(L):
    from csn_amd.minkowski_conv import build_kernel_map
    from csn_amd.minkowski_hrnet import build_pyramid
    rows = R.random_set(65, ts=2)
    cases = {"duplicate": (rows + [rows[3]], "coords holds duplicate rows"),
             "off_stride": (rows + [[0, 40, 41, 40]], "multiples of the tensor stride 2"),
             "batch": (rows + [[1 << 15, 40, 40, 40]], "batch indices must lie in"),
             "range": (rows + [[0, 40, 40, 32768]], "x, y, z must lie in")}
    for name, (bad, text) in cases.items():
        messages = []
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError, match=text) as err:
                build_kernel_map(_dev(bad), kernel_size=3, stride=1, tensor_stride=2, backend=backend)
            messages.append(str(err.value))
        assert messages[0] == messages[1], name
        messages = []
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError) as err:
                build_kernel_map(_dev(rows), kernel_size=3, stride=2, tensor_stride=1, out_coords=_dev(bad), backend=backend)
            messages.append(str(err.value))
        assert messages[0] == messages[1] and messages[0].startswith("out_coords"), name
    ones = R.random_set(65)
    for bad in (ones + [ones[0]], ones + [[1 << 15, 0, 0, 0]]):
        messages = []
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError) as err:
                build_pyramid(_dev(bad), 3, 5, backend=backend)
            messages.append(str(err.value))
        assert messages[0] == messages[1]
    with pytest.raises(ValueError, match="nonsense"):
        build_kernel_map(_dev(ones), backend="nonsense")


def _same_pyramid(a, b):
    assert a.n_levels == b.n_levels and a.stem_kernel == b.stem_kernel
    for l in range(a.n_levels):
        assert a.coords[l].dtype == torch.int64 and torch.equal(a.coords[l], b.coords[l])
        _same(a.s1[l], b.s1[l])
        assert a.s1[l].bwd_table is None
    _same(a.stem, b.stem)
    assert a.stem.bwd_table is None and (a.stem is a.s1[0]) == (b.stem is b.s1[0])
    for l in range(a.n_levels - 1):
        _same(a.down[l], b.down[l])
        assert a.down[l].bwd_table is not None
        for p in (a, b):                                                    # up(l) shares the tables of down[l]
            assert p.up(l).fwd is p.down[l].bwd_table and p.up(l).bwd_table is p.down[l].fwd and p.up(l).transposed
        _same(a.up(l), b.up(l))


@pytest.mark.parametrize("levels,stem", [(3, 5), (2, 3)])
@pytest.mark.parametrize("name", ["n1031", "two_clusters"])
def test_pyramids_are_indistinguishable(L, name, levels, stem):
    from csn_amd import tuning
    from csn_amd.minkowski_hrnet import build_pyramid
    coords = _dev(SETS[name](ts=1))
    ref = build_pyramid(coords, levels, stem, backend="torch")
    _same_pyramid(build_pyramid(coords, levels, stem, backend="hip"), ref)
    with tuning.override(native_kernel_maps=True):
        _same_pyramid(build_pyramid(coords, levels, stem), ref)


def test_the_native_pyramid_is_thirteen_library_calls_and_one_host_read(L, monkeypatch):
    from csn_amd import minkowski_conv as MC
    from csn_amd.minkowski_hrnet import build_pyramid
    coords = _dev(R.random_set(257))
    calls, reads = [], []
    read = MC._read_status
    monkeypatch.setattr(MC, "_read_status", lambda s: reads.append(1) or read(s))
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    try:
        build_pyramid(coords, 3, 5, backend="hip")
    finally:
        L.set_call_hook(None)
    assert sorted(calls) == ["csn_coord_down_i64"] * 2 + ["csn_coord_keys_i64"] * 3 + ["csn_kernel_map_i32"] * 8
    assert len(reads) == 1
    del calls[:], reads[:]
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    try:
        MC.build_kernel_map(coords, kernel_size=3, stride=2, backend="hip")
    finally:
        L.set_call_hook(None)
    assert calls == ["csn_coord_keys_i64", "csn_coord_down_i64", "csn_kernel_map_i32", "csn_kernel_map_i32"] and len(reads) == 1


def _by_shape(rows):
    return sorted(rows, key=lambda r: r[0])                                 # stable: the rows of a shape keep their random order


def test_a_training_step_has_the_same_bits_under_the_switch(L):
    """The tables are equal, so every launch downstream is the same launch: logits and every parameter gradient bit for bit.  (The
    attention's dropout seeds come from torch's CPU generator: every step is seeded alike.)"""
    from csn_amd import HRNetSimCSN2S, PointField, tuning
    torch.manual_seed(11)
    coords = _dev(_by_shape(R.random_set(257)))
    feats = torch.randn(257, 3, device="cuda")
    dy = torch.randn(257, 6, device="cuda")
    model = HRNetSimCSN2S(3, 6, d_model=64, n_head=2, k_neighbors=1, dropout=0.0).cuda().train()

    def step(native):
        m = copy.deepcopy(model)
        torch.manual_seed(23)
        calls = []
        L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
        try:
            with tuning.override(native_kernel_maps=native):
                logits = m((coords, feats))
                logits.backward(dy)
        finally:
            L.set_call_hook(None)
        assert ("csn_kernel_map_i32" in calls) == native
        return logits.detach(), [p.grad for p in m.parameters()], [b.clone() for b in m.buffers()]

    (y0, g0, b0), (y1, g1, b1) = step(False), step(True)
    assert torch.equal(y0, y1) and len(g0) == len(g1) and sum(g is not None for g in g0) > len(g0) // 2
    for a, b in zip(g0, g1):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))

    # the same through a point field: points inside the voxels, the pyramid asked for by name, logits interpolated back
    g = torch.Generator().manual_seed(5)
    pts = torch.cat([coords[:, :1].float(), coords[:, 1:].float() + torch.rand(257, 3, generator=g).cuda() * 0.9 + 0.05], dim=1).repeat(2, 1)
    pts = pts[torch.argsort(pts[:, 0], stable=True)].contiguous()
    pf = torch.randn(pts.shape[0], 3, device="cuda")
    dp = torch.randn(pts.shape[0], 6, device="cuda")

    def field_step(backend):
        m = copy.deepcopy(model)
        torch.manual_seed(29)
        field = PointField(pts, pf)
        assert field.n_voxels == 257
        pyr = field.pyramid(2, backend=backend)
        assert field.corner_table(backend=backend) is pyr.s1[0].fwd
        out = field.interpolate(m(field.sparse()))
        out.backward(dp)
        return out.detach(), [p.grad for p in m.parameters()]

    (y0, g0), (y1, g1) = field_step("torch"), field_step("hip")
    assert torch.equal(y0, y1)
    for a, b in zip(g0, g1):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
