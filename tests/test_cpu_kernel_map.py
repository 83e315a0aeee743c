"""CPU-side checks (no GPU needed) of the native kernel-map backend (include/csn_hip.h section 17, csrc/kernel_map.hip): the three
entry points refuse bad arguments on the host with the documented codes, the Python surface routes CPU tensors to the torch backend
(or refuses them where ``"hip"`` is asked for by name), and every kernel of the new file compiles for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import sparse_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, PTR, DIM = -1, -3, -5


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    return csn_amd.lib()


def test_entry_points_validate_on_the_host(L):
    """The non-NULL pointers are host buffers that are never dereferenced: every call below returns before any launch."""
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    keys = lambda co=p, n=3, ts=1, k=p, st=p: L.csn_coord_keys_i64(co, n, ts, k, st, None)
    down = lambda k=p, n=3, ts=2, d=p: L.csn_coord_down_i64(k, n, ts, d, None)
    kmap = lambda sk=p, sr=p, ns=3, qk=p, nq=2, ks=3, step=1, tab=p, st=p: L.csn_kernel_map_i32(sk, sr, ns, qk, nq, ks, step, tab, st, None)
    for name in ("co", "k", "st"):
        assert keys(**{name: None}) == ARG, name
    for name in ("k", "d"):
        assert down(**{name: None}) == ARG, name
    for name in ("sk", "qk", "tab", "st"):
        assert kmap(**{name: None}) == ARG, name
    for fn in (keys, down):
        assert fn(n=0) == ARG and fn(n=-4) == ARG and fn(ts=0) == ARG and fn(ts=-2) == ARG
    assert kmap(ns=0) == ARG and kmap(nq=0) == ARG and kmap(ns=-1) == ARG and kmap(nq=-1) == ARG
    assert kmap(step=0) == ARG
    for ks in (2, 7, 0, -3, 4):
        assert kmap(ks=ks) == DIM, ks
    assert kmap(ks=2, step=0) == ARG                                       # a bad argument is named before a bad kernel size
    # a key or coordinate array off 8 bytes, an int32 array or the status word off 4
    assert keys(co=p + 4) == PTR and keys(k=p + 4) == PTR and keys(st=p + 2) == PTR
    assert down(k=p + 4) == PTR and down(d=p + 1) == PTR
    assert kmap(sk=p + 4) == PTR and kmap(qk=p + 4) == PTR and kmap(tab=p + 2) == PTR and kmap(st=p + 1) == PTR and kmap(sr=p + 2) == PTR
    assert kmap(sk=p + 4, ks=7) == DIM                                     # ... and a bad kernel size before a bad pointer


def test_the_switch_is_off_by_default():
    from csn_amd import tuning
    assert tuning.Tuning().native_kernel_maps is False and tuning.current().native_kernel_maps is False
    with tuning.override(native_kernel_maps=True) as t:
        assert t.native_kernel_maps is True and tuning.current().native_kernel_maps is True
    assert tuning.current().native_kernel_maps is False


def _same_map(a, b):
    assert torch.equal(a.in_coords, b.in_coords) and torch.equal(a.out_coords, b.out_coords) and torch.equal(a.fwd, b.fwd)
    assert (a.bwd_table is None) == (b.bwd_table is None) and torch.equal(a.bwd, b.bwd)
    assert a.fwd.dtype == b.fwd.dtype == torch.int32 and a.out_coords.dtype == b.out_coords.dtype == torch.int64
    assert (a.kernel_size, a.stride, a.in_tensor_stride, a.out_tensor_stride, a.transposed) == \
           (b.kernel_size, b.stride, b.in_tensor_stride, b.out_tensor_stride, b.transposed)


def test_cpu_tensors_keep_the_torch_backend():
    from csn_amd import CsnError, PointField, tuning
    from csn_amd.minkowski_conv import build_kernel_map
    from csn_amd.minkowski_hrnet import build_pyramid
    coords = torch.tensor(R.random_set(65))
    fine = torch.tensor(R.random_set(63, ts=1, seed=3))
    for kw in (dict(kernel_size=5), dict(stride=2), dict(stride=2, tensor_stride=2, out_coords=fine, transposed=True)):
        c = coords * torch.tensor([1, 2, 2, 2]) if kw.get("transposed") else coords
        with pytest.raises(CsnError, match="no CPU path"):
            build_kernel_map(c, backend="hip", **kw)
        with pytest.raises(ValueError, match="nonsense"):
            build_kernel_map(c, backend="nonsense", **kw)
        ref = build_kernel_map(c, **kw)
        _same_map(build_kernel_map(c, backend="torch", **kw), ref)
        with tuning.override(native_kernel_maps=True):                       # the switch alone never sends CPU tensors to the library
            _same_map(build_kernel_map(c, **kw), ref)
    with pytest.raises(CsnError, match="no CPU path"):
        build_pyramid(coords, 2, 3, backend="hip")
    with pytest.raises(ValueError, match="nonsense"):
        build_pyramid(coords, 2, 3, backend="nonsense")
    ref = build_pyramid(coords, 2, 5)
    with tuning.override(native_kernel_maps=True):
        for pyr in (build_pyramid(coords, 2, 5, backend="torch"), build_pyramid(coords, 2, 5)):
            assert all(torch.equal(a, b) for a, b in zip(pyr.coords, ref.coords)) and pyr.n_levels == 2
            _same_map(pyr.s1[0], ref.s1[0]), _same_map(pyr.s1[1], ref.s1[1]), _same_map(pyr.stem, ref.stem), _same_map(pyr.down[0], ref.down[0])
    pts = torch.cat([coords[:, :1].float(), coords[:, 1:].float() + 0.25], dim=1)
    pts = pts[torch.argsort(pts[:, 0], stable=True)]
    field = PointField(pts, torch.zeros(pts.shape[0], 1))
    with pytest.raises(CsnError, match="no CPU path"):
        field.pyramid(2, backend="hip")
    with pytest.raises(CsnError, match="no CPU path"):
        field.corner_table(backend="hip")
    assert torch.equal(field.pyramid(2, backend="torch").s1[0].fwd, build_kernel_map(field.voxel_coords).fwd)


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_kernel_map_kernels_use_no_scratch_and_no_lds(tmp_path):
    from csn_amd import _lib
    flags = [f for f in _lib.BUILD_FLAGS if f != "-shared"]
    res = subprocess.run([_hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csn_amd", "csrc", "kernel_map.hip"),
                          "-o", str(tmp_path / "kernel_map.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = []
    for b in re.split(r"Function Name: ", res.stderr)[1:]:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)E", b)
        assert m, b[:200]
        field = lambda key: int(re.search(re.escape(key) + r":? (\d+)", b).group(1))
        assert field("ScratchSize [bytes/lane]") == 0, m.group(1)
        assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, m.group(1)
        assert field("LDS Size [bytes/block]") == 0, m.group(1)
        assert field("Occupancy [waves/SIMD]") == 8, m.group(1)
        seen.append(m.group(1))
    assert sorted(seen) == ["coord_down_kernel", "coord_keys_kernel", "kernel_map_kernel"]
