"""The native octant-map backend on the MI355X (include/csn_hip.h section 22, csrc/octant_map.hip; ``backend="hip"`` of
csn_amd.minkowski_conv.build_octant_map and csn_amd.minkowski_unet.build_unet_pyramid) against two references that are not the code
under test: the torch backend on the same device tensors (``torch.equal`` on every attribute — the results are integers, there is
no tolerance) and the dictionary restatement ``tests/octant_ref.Partition``.  The raw entry points always write into the middle of
larger buffers filled with a sentinel, and the margins are looked at after every call."""
import copy

import numpy as np
import pytest
import torch

from tests import octant_ref as O
from tests import sparse_conv_ref as R
from tests.test_gpu_kernel_map import SETS, _same

pytestmark = pytest.mark.gpu

CANARY = -777
PAD = 70
ALL_SETS = {**SETS, "even_y": O.even_y}
OMAP_TENSORS = ("in_coords", "out_coords", "parent", "octant", "children", "order", "seg")


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


def _same_omap(a, b):
    """Two ``OctantMap`` objects are indistinguishable."""
    for name in OMAP_TENSORS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), name
        assert x.is_contiguous() and x.dtype == (torch.int64 if name.endswith("coords") else torch.int32), name
    assert (a.in_tensor_stride, a.out_tensor_stride, a.n_fine, a.n_coarse) == (b.in_tensor_stride, b.out_tensor_stride, b.n_fine, b.n_coarse)


def _is_partition(m, p):
    assert m.parent.tolist() == p.parent and m.octant.tolist() == p.octant and m.children.tolist() == p.children
    assert m.out_coords.tolist() == [list(c) for c in p.coarse]
    assert m.order.tolist() == sorted(range(p.n_fine), key=lambda i: (p.octant[i], i))
    assert m.seg.tolist() == [sum(p.segments()[:k]) for k in range(9)]


def _both(rows, ts, out=None):
    from csn_amd.minkowski_conv import build_octant_map
    kw = dict(tensor_stride=ts, out_coords=None if out is None else _dev(out))
    hip, ref = build_octant_map(_dev(rows), backend="hip", **kw), build_octant_map(_dev(rows), backend="torch", **kw)
    _same_omap(hip, ref)
    _is_partition(hip, O.Partition(rows, ts, out))
    return hip


@pytest.mark.parametrize("ts", [1, 2, 8])
@pytest.mark.parametrize("name", list(ALL_SETS))
def test_every_set_equals_the_torch_backend_and_the_partition(L, name, ts):
    rows = ALL_SETS[name](ts=ts)
    if name == "two_clusters":                       # its line of isolated voxels leaves the packed range at ts = 8: 102 of 139 stay
        rows = [r for r in rows if max(r[1:]) < 32768]
        assert len(rows) > 200
    rows = _shuffled(rows, 4)
    assert min(min(r[1:]) for r in rows) < 0                                                    # negative coordinates are there
    m = _both(rows, ts)
    _both(rows, ts, out=_shuffled(m.out_coords.tolist(), 5))                                    # onto a given, shuffled coarse set
    if name == "even_y":
        assert sum(m.seg[k + 1].item() == m.seg[k].item() for k in range(8)) == 4               # four empty octants


# ------------------------------------------------------------------------------------------------------
# the raw entry points, inside sentinel margins
# ------------------------------------------------------------------------------------------------------
def _inside(n, dtype=torch.int32):
    buf = torch.full((PAD + n + PAD,), CANARY, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _margins_hold(*bufs):
    for buf in bufs:
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def _raw_partition(L, fine_keys, ts, coarse_keys, coarse_rows=None, fine_sorted=None):
    n_fine, n_coarse = fine_keys.numel(), coarse_keys.numel()
    (pb, parent), (ob, octant), (cb, children) = _inside(n_fine), _inside(n_fine), _inside(8 * n_coarse)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(L.lib().csn_octant_partition_i32(ptr(fine_keys), ptr(fine_sorted), n_fine, ts, ptr(coarse_keys), ptr(coarse_rows), n_coarse,
                                             ptr(parent), ptr(octant), ptr(children), ptr(status), torch.cuda.current_stream().cuda_stream),
            "csn_octant_partition_i32")
    word = status.item()
    _margins_hold(pb, ob, cb)
    return parent, octant, children.view(8, n_coarse), word


def _raw_order(L, octant):
    n = octant.numel()
    (rb, order), (sb, seg) = _inside(n), _inside(9)
    ws_n = L.lib().csn_octant_order_workspace_bytes(n)
    wb, ws = _inside(ws_n // 4)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.lib().csn_octant_order_i32(octant.data_ptr(), n, order.data_ptr(), seg.data_ptr(), ws.data_ptr(), ws_n, status.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "csn_octant_order_i32")
    word = status.item()
    _margins_hold(rb, sb, wb)
    return order, seg, word


def _sorted_order(octant):
    """order and seg of the torch backend for a VALID octant array."""
    seg = torch.zeros(9, dtype=torch.int32, device=octant.device)
    seg[1:] = torch.cumsum(torch.bincount(octant, minlength=8), 0).int()
    return torch.sort(octant, stable=True)[1].int(), seg


def _raw_map_equals_the_torch_backend(L, rows, ts=1):
    from csn_amd.minkowski_conv import _pack, build_octant_map
    ref = build_octant_map(_dev(rows), tensor_stride=ts, backend="torch")
    parent, octant, children, word = _raw_partition(L, _pack(_dev(rows)), ts, _pack(ref.out_coords))
    assert word == 0 and torch.equal(parent, ref.parent) and torch.equal(octant, ref.octant) and torch.equal(children, ref.children)
    order, seg, word = _raw_order(L, octant.contiguous())
    assert word == 0 and torch.equal(order, ref.order) and torch.equal(seg, ref.seg)
    return ref


def _edge_sizes():
    from csn_amd.minkowski_conv import OCTANT_ORDER_TILE as T
    return sorted({1, 63, 64, 65, 255, 256, 257, 1031, T - 1, T, T + 1})


def test_the_sizes_at_the_edges_of_the_kernels_loops(L):
    rows = R.random_set(1031)
    for n in _edge_sizes():
        _raw_map_equals_the_torch_backend(L, rows[:n])


def test_the_scan_covers_more_tiles_than_one_pass_of_its_work_group(L):
    from csn_amd.minkowski_conv import OCTANT_ORDER_SCAN as W, OCTANT_ORDER_TILE as T
    n = T * W + T + 37                                                     # W + 2 tiles, the last one partial
    g = torch.Generator().manual_seed(3)
    octant = torch.randint(0, 8, (n,), generator=g, dtype=torch.int32).cuda()
    order, seg, word = _raw_order(L, octant)
    want_order, want_seg = _sorted_order(octant)
    assert word == 0 and torch.equal(seg, want_seg) and torch.equal(order, want_order)
    order2, seg2, _ = _raw_order(L, octant)                                # identical on every call
    assert torch.equal(order, order2) and torch.equal(seg, seg2)


def test_one_octant_two_octants_and_one_parent(L):
    base = R.random_set(257)
    even = [[b, 2 * x, 2 * y, 2 * z] for b, x, y, z in base]
    ref = _raw_map_equals_the_torch_backend(L, even)                       # every row in octant 0
    assert ref.seg.tolist() == [0] + [257] * 8
    odd = [[b, x + 1, y + 1, z + 1] for b, x, y, z in even]
    ref = _raw_map_equals_the_torch_backend(L, odd)                        # every row in octant 7
    assert ref.seg.tolist() == [0] * 8 + [257]
    ref = _raw_map_equals_the_torch_backend(L, even[:130] + odd[130:])     # octants 0 and 7 only
    assert ref.seg.tolist() == [0] + [130] * 7 + [257]
    cell = [[3, -6 + x, 10 + y, -2 + z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    for rows in (cell, cell[5:] + cell[:2], cell[6:7]):                    # n_coarse = 1
        ref = _raw_map_equals_the_torch_backend(L, rows)
        assert ref.n_coarse == 1 and ref.parent.tolist() == [0] * len(rows)
    ref = _raw_map_equals_the_torch_backend(L, [[b, 8 * x, 8 * y, 8 * z] for b, x, y, z in cell], ts=8)
    assert ref.n_coarse == 1 and sorted(ref.octant.tolist()) == list(range(8))


def test_the_search_ends_inside_its_array_at_both_ends_and_a_missing_parent_is_flagged(L):
    """The coarse set is a VIEW inside a larger key buffer whose neighbours hold exactly the parents some fine rows ask for: those
    rows read "no parent" (flag 16, parent -1, no children entry), which a search that looked one element outside its array would
    not; the rows whose parent is the view's first or last key find it."""
    from csn_amd.minkowski_conv import _pack
    rows = R.random_set(257)
    p = O.Partition(rows)
    last = p.n_coarse - 1
    assert {0, 1, last - 1, last} <= set(p.parent)
    buf = _pack(_dev([list(c) for c in p.coarse]))
    parent, octant, children, word = _raw_partition(L, _pack(_dev(rows)), 1, buf[1:-1])
    want = [j - 1 if 1 <= j < last else -1 for j in p.parent]
    assert word == 16 and parent.tolist() == want and octant.tolist() == p.octant
    assert children.tolist() == [c[1:-1] for c in p.children]
    # the coarse rows in another order (coarse_rows), the same gap: a row number is taken from the array, a missing parent is still -1
    perm = torch.randperm(last - 1, generator=torch.Generator().manual_seed(1)).int().cuda()
    parent, _, children, word = _raw_partition(L, _pack(_dev(rows)), 1, buf[1:-1], coarse_rows=perm)
    assert word == 16 and parent.tolist() == [-1 if j < 0 else perm[j].item() for j in want]
    kids = torch.full((8, last - 1), -1, dtype=torch.int32)
    for i, (j, k) in enumerate(zip(parent.tolist(), p.octant)):
        if j >= 0:
            kids[k, j] = i
    assert torch.equal(children.cpu(), kids)
    # a coarse_rows entry outside [0, n_coarse) reads as "no parent" and is not followed
    bad = perm.clone()
    bad[0], bad[1] = last - 1, -1
    parent, _, _, word = _raw_partition(L, _pack(_dev(rows)), 1, buf[1:-1], coarse_rows=bad)
    assert word == 16 and all(-1 <= j < last - 1 for j in parent.tolist())


def test_sets_that_do_not_ascend_are_flagged(L):
    from csn_amd.minkowski_conv import _pack
    rows = R.random_set(257)
    p = O.Partition(rows)
    keys, coarse = _pack(_dev(rows)), _pack(_dev([list(c) for c in p.coarse]))
    assert _raw_partition(L, keys, 1, coarse, fine_sorted=torch.sort(keys)[0])[3] == 0
    assert _raw_partition(L, keys, 1, coarse.flip(0).contiguous())[3] & 8                       # a descending coarse set
    twice = torch.cat([coarse[:70], coarse[69:]])                                               # a duplicate coarse row
    assert _raw_partition(L, keys, 1, twice)[3] == 8
    for at in (0, 63, 255):                                                                     # a duplicate fine row, in any wave
        dup = torch.cat([keys, keys[at:at + 1]])
        parent, octant, _, word = _raw_partition(L, dup, 1, coarse, fine_sorted=torch.sort(dup)[0])
        assert word == 8 and parent.tolist() == p.parent + [p.parent[at]] and octant.tolist() == p.octant + [p.octant[at]]


@pytest.mark.parametrize("n", [5, 257, 1031])
def test_an_octant_entry_outside_its_range_is_dropped_and_flagged(L, n):
    g = torch.Generator().manual_seed(n)
    octant = torch.randint(0, 8, (n,), generator=g, dtype=torch.int32)
    bad = {0: 9, n // 2: -1, n - 1: 8, n // 3: 1 << 30}
    for i, v in bad.items():
        octant[i] = v
    octant = octant.cuda()
    order, seg, word = _raw_order(L, octant)
    keep = torch.tensor([i for i in range(n) if i not in bad], device="cuda")
    want_order, want_seg = _sorted_order(octant[keep])
    kept = n - len(bad)
    assert word == 32 and torch.equal(seg, want_seg) and seg[8].item() == kept
    assert torch.equal(order[:kept], keep[want_order.long()].int()) and bool((order[kept:] == CANARY).all())


def test_bad_coordinates_raise_the_torch_backends_messages(L):
    from csn_amd.minkowski_conv import build_octant_map
    rows = R.random_set(65, ts=2)
    coarse = O.Partition(rows, 2).coarse
    good_out = [list(c) for c in coarse]
    cases = {"range": (rows + [[0, 40, 40, 32768]], None, "coords: x, y, z must lie in"),
             "batch": (rows + [[1 << 15, 40, 40, 40]], None, "coords: batch indices must lie in"),
             "off_stride": (rows + [[0, 40, 41, 40]], None, "coords: x, y, z must be multiples of the tensor stride 2"),
             "duplicate": (rows + [rows[3]], None, "coords holds duplicate rows"),
             "duplicate_given": (rows + [rows[3]], good_out, "coords holds duplicate rows"),
             "out_duplicate": (rows, good_out + [good_out[2]], "out_coords holds duplicate rows"),
             "out_off_stride": (rows, good_out + [[0, 400, 402, 400]], "out_coords: x, y, z must be multiples of the tensor stride 4"),
             "out_range": (rows, good_out + [[0, 400, 400, -32772]], "out_coords: x, y, z must lie in"),
             "missing_parent": (rows, good_out[:-1], "out_coords misses the parent of some row of coords"),
             "missing_first_parent": (rows, good_out[1:], "out_coords misses the parent of some row of coords")}
    for name, (fine, out, text) in cases.items():
        messages = []
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError) as err:
                build_octant_map(_dev(fine), tensor_stride=2, out_coords=None if out is None else _dev(_shuffled(out, 2)), backend=backend)
            messages.append(str(err.value))
        assert messages[0] == messages[1] and messages[0].startswith(text), (name, messages)
    with pytest.raises(ValueError, match="nonsense"):
        build_octant_map(_dev(rows), tensor_stride=2, backend="nonsense")
    with pytest.raises(ValueError, match="tensor_stride 0"):
        build_octant_map(_dev(rows), tensor_stride=0, backend="hip")


# ------------------------------------------------------------------------------------------------------
# the pyramid
# ------------------------------------------------------------------------------------------------------
def _same_unet_pyramid(a, b):
    assert a.stem_kernel == b.stem_kernel and len(a.coords) == len(b.coords) == 5
    assert len(a.s1) == len(a.one) == 5 and len(a.oct) == 4
    for l in range(5):
        assert a.coords[l].dtype == torch.int64 and torch.equal(a.coords[l], b.coords[l])
        for x, y, k in ((a.s1[l], b.s1[l], 3), (a.one[l], b.one[l], 1)):
            _same(x, y)
            assert x.bwd_table is None and x.kernel_size == k and x.in_tensor_stride == 1 << l
    _same(a.stem, b.stem)
    assert a.stem.bwd_table is None and (a.stem is a.s1[0]) == (b.stem is b.s1[0])
    for l in range(4):
        _same_omap(a.oct[l], b.oct[l])
        assert a.oct[l].in_tensor_stride == 1 << l and torch.equal(a.oct[l].out_coords, a.coords[l + 1])


def _points_in(coords):
    """Points inside the voxels ``coords`` (sorted by shape), two per voxel."""
    g = torch.Generator().manual_seed(5)
    n = coords.shape[0]
    pts = torch.cat([coords[:, :1].float(), coords[:, 1:].float() + torch.rand(n, 3, generator=g).cuda() * 0.9 + 0.05], dim=1).repeat(2, 1)
    return pts[torch.argsort(pts[:, 0], stable=True)].contiguous()


@pytest.mark.parametrize("stem", [5, 3])
@pytest.mark.parametrize("name", ["n1031", "two_clusters"])
def test_pyramids_are_indistinguishable(L, name, stem):
    from csn_amd import PointField, tuning
    from csn_amd.minkowski_unet import build_unet_pyramid
    coords = _dev(SETS[name](ts=1))
    ref = build_unet_pyramid(coords, stem, backend="torch")
    _same_unet_pyramid(build_unet_pyramid(coords, stem, backend="hip"), ref)
    with tuning.override(native_kernel_maps=True):
        _same_unet_pyramid(build_unet_pyramid(coords, stem), ref)
    pts = _points_in(coords)
    field = PointField(pts, torch.zeros(pts.shape[0], 1, device="cuda"))
    ref = build_unet_pyramid(field.voxel_coords, stem, backend="torch")
    pyr = field.unet_pyramid(stem, backend="hip")
    _same_unet_pyramid(pyr, ref)
    assert field.unet_pyramid(stem) is pyr and field.corner_table() is pyr.s1[0].fwd and field.sparse()[0] is field.voxel_coords


def _calls_and_reads(L, monkeypatch, fn):
    from csn_amd import minkowski_conv as MC
    calls, reads = [], []
    read = MC._read_status
    monkeypatch.setattr(MC, "_read_status", lambda s: reads.append(1) or read(s))
    L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
    try:
        fn()
    finally:
        L.set_call_hook(None)
        monkeypatch.setattr(MC, "_read_status", read)
    return calls, len(reads)


def test_the_native_pyramid_is_twenty_eight_library_calls_and_one_host_read(L, monkeypatch):
    from csn_amd import minkowski_conv as MC
    from csn_amd.minkowski_unet import build_unet_pyramid
    coords = _dev(R.random_set(257))
    calls, reads = _calls_and_reads(L, monkeypatch, lambda: build_unet_pyramid(coords, 5, backend="hip"))
    assert sorted(calls) == (["csn_coord_down_i64"] * 4 + ["csn_coord_keys_i64"] * 5 + ["csn_kernel_map_i32"] * 11 +
                             ["csn_octant_order_i32"] * 4 + ["csn_octant_partition_i32"] * 4) and reads == 1
    calls, reads = _calls_and_reads(L, monkeypatch, lambda: build_unet_pyramid(coords, 3, backend="hip"))
    assert len(calls) == 27 and calls.count("csn_kernel_map_i32") == 10 and reads == 1
    calls, reads = _calls_and_reads(L, monkeypatch, lambda: MC.build_octant_map(coords, backend="hip"))
    assert calls == ["csn_coord_keys_i64", "csn_coord_down_i64", "csn_octant_partition_i32", "csn_octant_order_i32"] and reads == 1
    out = _dev(_shuffled(O.Partition(coords.tolist()).coarse, 1))
    calls, reads = _calls_and_reads(L, monkeypatch, lambda: MC.build_octant_map(coords, out_coords=out, backend="hip"))
    assert calls == ["csn_coord_keys_i64", "csn_coord_keys_i64", "csn_octant_partition_i32", "csn_octant_order_i32"] and reads == 1


def test_a_training_step_has_the_same_bits_under_the_switch(L):
    """The maps are equal, so every launch downstream is the same launch: logits and every parameter gradient bit for bit."""
    from csn_amd import Res16UNet14A, tuning
    torch.manual_seed(11)
    coords = _dev(sorted(R.random_set(257), key=lambda r: r[0]))
    feats = torch.randn(257, 3, device="cuda")
    labels = torch.randint(0, 6, (257,), device="cuda")
    model = Res16UNet14A(3, 6).cuda().train()

    def step(native):
        m = copy.deepcopy(model)
        calls = []
        L.set_call_hook(lambda name, phase: calls.append(name) if phase == "begin" else None)
        try:
            with tuning.override(native_kernel_maps=native):
                logits = m((coords, feats))
                torch.nn.functional.cross_entropy(logits, labels).backward()
        finally:
            L.set_call_hook(None)
        assert ("csn_octant_partition_i32" in calls) == native and ("csn_kernel_map_i32" in calls) == native
        return logits.detach(), [p.grad for p in m.parameters()], [b.clone() for b in m.buffers()]

    (y0, g0, b0), (y1, g1, b1) = step(False), step(True)
    assert torch.equal(y0, y1) and len(g0) == len(g1) and sum(g is not None for g in g0) > len(g0) // 2
    for a, b in zip(g0, g1):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))
