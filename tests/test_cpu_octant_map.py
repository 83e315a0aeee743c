"""CPU-side checks (no GPU needed) of the native octant-map backend (include/csn_hip.h section 22, csrc/octant_map.hip): the entry
points refuse bad arguments on the host with the documented codes, the Python surface keeps CPU tensors on the torch backend (or
refuses them where ``"hip"`` is asked for by name), the default path still gives the integers of ``tests/octant_ref.Partition``,
and the constants the Python side states for the order kernel are the library's."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import octant_ref as O
from tests import sparse_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, PTR, WORKSPACE = -1, -3, -6


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    return csn_amd.lib()


def test_entry_points_validate_on_the_host(L):
    """The non-NULL pointers are host buffers that are never dereferenced: every call below returns before any launch."""
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    part = lambda fk=p, fs=p, nf=3, ts=1, ck=p, cr=p, nc=2, par=p, oc=p, ch=p, st=p: \
        L.csn_octant_partition_i32(fk, fs, nf, ts, ck, cr, nc, par, oc, ch, st, None)
    need = L.csn_octant_order_workspace_bytes(3)
    order = lambda oc=p, n=3, od=p, sg=p, ws=p, nb=need, st=p: L.csn_octant_order_i32(oc, n, od, sg, ws, nb, st, None)
    for name in ("fk", "ck", "par", "oc", "ch", "st"):
        assert part(**{name: None}) == ARG, name
    for name in ("oc", "od", "sg", "ws", "st"):
        assert order(**{name: None}) == ARG, name
    for bad in (0, -4):
        assert part(nf=bad) == ARG and part(nc=bad) == ARG and part(ts=bad) == ARG and order(n=bad) == ARG
    # a key array off 8 bytes; an int32 array, the workspace or the status word off 4
    for name in ("fk", "fs", "ck"):
        assert part(**{name: p + 4}) == PTR, name
    for name in ("cr", "par", "oc", "ch", "st"):
        assert part(**{name: p + 2}) == PTR, name
    for name in ("oc", "od", "sg", "ws", "st"):
        assert order(**{name: p + 2}) == PTR, name
    assert part(fk=p + 4, nf=0) == ARG                                     # a bad argument is named before a bad pointer
    assert order(nb=need - 1) == WORKSPACE and order(nb=0) == WORKSPACE and order(ws=p + 2, nb=0) == PTR


def test_the_workspace_is_eight_counts_per_tile_of_the_stated_size(L):
    from csn_amd import minkowski_conv as MC
    src = open(os.path.join(ROOT, "csn_amd", "csrc", "csn_kernels.h")).read()
    T = int(re.search(r"CSN_OCTANT_ORDER_TILE = (\d+);", src).group(1))
    W = int(re.search(r"CSN_OCTANT_ORDER_SCAN = (\d+);", src).group(1))
    assert (MC.OCTANT_ORDER_TILE, MC.OCTANT_ORDER_SCAN) == (T, W)
    for n, tiles in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (T * W + 1, W + 1), (2 ** 31 - 1, (2 ** 31 - 1 + T - 1) // T)):
        assert L.csn_octant_order_workspace_bytes(n) == 32 * tiles, n
    assert L.csn_octant_order_workspace_bytes(0) == 0 and L.csn_octant_order_workspace_bytes(-5) == 0


def _same_octant_map(m, p, ts):
    assert m.in_tensor_stride == ts and m.out_tensor_stride == 2 * ts
    assert m.parent.tolist() == p.parent and m.octant.tolist() == p.octant and m.children.tolist() == p.children
    assert m.out_coords.tolist() == [list(c) for c in p.coarse]
    order = sorted(range(p.n_fine), key=lambda i: (p.octant[i], i))
    assert m.order.tolist() == order
    assert m.seg.tolist() == [sum(p.segments()[:k]) for k in range(9)]
    for t in (m.parent, m.octant, m.children, m.order, m.seg):
        assert t.dtype == torch.int32


def test_cpu_tensors_keep_the_torch_backend_and_the_default_path_is_the_partition():
    from csn_amd import CsnError, PointField, tuning
    from csn_amd.minkowski_conv import build_octant_map
    from csn_amd.minkowski_unet import build_unet_pyramid
    for rows, ts in ((R.random_set(65), 1), (O.even_y(63, ts=2), 2)):
        coords = torch.tensor(rows)
        p = O.Partition(rows, ts)
        given = [list(c) for c in reversed(p.coarse)]
        for out in (None, given):
            kw = dict(tensor_stride=ts, out_coords=None if out is None else torch.tensor(out))
            want = p if out is None else O.Partition(rows, ts, out)
            _same_octant_map(build_octant_map(coords, **kw), want, ts)                   # the default path, as before
            _same_octant_map(build_octant_map(coords, backend="torch", **kw), want, ts)
            with tuning.override(native_kernel_maps=True):                               # the switch alone never sends CPU tensors to the library
                _same_octant_map(build_octant_map(coords, **kw), want, ts)
            with pytest.raises(CsnError, match="no CPU path"):
                build_octant_map(coords, backend="hip", **kw)
            with pytest.raises(ValueError, match="nonsense"):
                build_octant_map(coords, backend="nonsense", **kw)
    coords = torch.tensor(R.random_set(65))
    with pytest.raises(CsnError, match="no CPU path"):
        build_unet_pyramid(coords, 3, backend="hip")
    with pytest.raises(ValueError, match="nonsense"):
        build_unet_pyramid(coords, 3, backend="nonsense")
    ref = build_unet_pyramid(coords, 3)
    with tuning.override(native_kernel_maps=True):
        pyr = build_unet_pyramid(coords, 3)
    for l in range(4):
        assert torch.equal(pyr.oct[l].children, ref.oct[l].children) and torch.equal(pyr.coords[l + 1], ref.coords[l + 1])
        _same_octant_map(ref.oct[l], O.Partition(ref.coords[l].tolist(), 1 << l), 1 << l)
    pts = torch.cat([coords[:, :1].float(), coords[:, 1:].float() + 0.25], dim=1)
    pts = pts[torch.argsort(pts[:, 0], stable=True)]
    field = PointField(pts, torch.zeros(pts.shape[0], 1))
    with pytest.raises(CsnError, match="no CPU path"):
        field.unet_pyramid(backend="hip")
    kept = field.unet_pyramid(3, backend="torch")
    assert field.unet_pyramid(3) is kept and field.unet_pyramid(5) is not kept           # built once and kept per stem kernel
    assert field.sparse()[0] is field.voxel_coords                                       # sparse() is as it was


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_octant_map_kernels_use_no_scratch_and_only_the_ballot_counts_in_lds(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", "octant_map.hip"),
                          "-o", str(tmp_path / "octant_map.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lds = {}
    for b in re.split(r"Function Name: ", res.stderr)[1:]:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)E", b)
        assert m, b[:200]
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        assert field("ScratchSize [bytes/lane]") == 0, m.group(1)
        assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, m.group(1)
        assert field("Occupancy [waves/SIMD]") == 8, m.group(1)
        lds[m.group(1)] = field("LDS Size [bytes/block]")
    # the partition keeps nothing in LDS; count and scatter their waves' eight counts, the scan its waves' totals
    assert lds == {"octant_partition_kernel": 0, "octant_count_kernel": 128, "octant_scan_kernel": 16, "octant_scatter_kernel": 128}
