"""Point fields: from the points of a batch to voxel rows, and from voxel logits back to the points, on the MI355X kernels.

Reference (marios2019/CSN):
  * ``Trainer._fetch_data``: ``ME.TensorField(features, coordinates, quantization_mode=...)``, ``field.sparse()``
                                                                                    MinkowskiNet/lib/trainer_csn.py:236-260
  * ``soutput.interpolate(queries_field)`` before the loss and the metrics           MinkowskiNet/lib/trainer_csn.py:200-205, 463-471
  * ``construct_shape_graph`` builds its inputs the same way                         MinkowskiNet/lib/csn_utils.py:52-80
  * the default ``quantization_mode`` ("random_subsample")                           MinkowskiNet/lib/config.py:159-162

The reference's loss, precision and IoUs are computed on POINT rows: the network sees the voxels of a batch, its logits are
interpolated back onto the points.  ``PointField`` is both halves.  What follows is THIS PROJECT'S statement of what MinkowskiEngine
does (MinkowskiEngine cannot be imported on this platform): parity unpinned against MinkowskiEngine, like the offset numbering of
minkowski_conv.py.

  * points        ``coords (Np, 4)`` float32 ``[b, x, y, z]`` in voxel units (the reference's ``Voxelizer`` has already divided by the
                  voxel size), ``b`` integral and non-decreasing; ``feats (Np, Cf)`` float32.  NaN / inf, or a floor outside the
                  packed range of minkowski_conv.py, raises ``ValueError``.
  * quantisation  the home voxel of a point is ``[b, floor(x), floor(y), floor(z)]`` (floor, not truncation: -0.3 -> -1).  The voxel
                  rows are the unique home voxels sorted by (b, x, y, z) at tensor stride 1: sorted by shape, as ``HRNetSimCSN``
                  wants them.  ``"random_subsample"``: a voxel takes the features of its LOWEST-NUMBERED point (MinkowskiEngine's
                  pick is an accident of its hash insert; ours is fixed).  ``"unweighted_average"``: the mean over the voxel's points,
                  added in point order.
  * interpolation of a map ``z (Nv, C)`` on the field's own voxel rows: ``t = xyz - floor(xyz)`` — the fp32 difference, which is
                  exact except for x in (-0.5, 0), where the true difference has no fp32 form and t is its rounding (still in
                  [0, 1]); that t is the definition —
                      y[p] = sum_{c in {0,1}^3} w_c(p) z[row(home(p) + c)],   w_c = prod_i (c_i ? t_i : 1 - t_i).
                  A corner with no voxel contributes nothing and the weights are NOT renormalised; corners never cross batch
                  indices.  On the dense volume that holds the voxel set and zeros elsewhere this is torch's
                  ``grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True)``.
  * gradient      the exact adjoint ``dz[v] = sum_c sum_{p : home(p) = v - c} w_c(p) dy[p]``; nothing flows to the coordinates.

The index arrays are plumbing in torch ops, device or CPU tensors alike (one stable sort of the packed keys,
``unique_consecutive``, a cumsum), like ``build_kernel_map``.  The field keeps NO corner tables: the kernel-3 stride-1 map of level 0
(``VoxelPyramid.s1[0].fwd``) already holds the row of ``v + c`` at ``fwd[13 + cx + 3 cy + 9 cz][v]`` and of ``v - c`` at
``fwd[13 - cx - 3 cy - 9 cz][v]``.  The arithmetic is include/csn_hip.h section 16: ``csn_voxel_mean_f32``,
``csn_point_interp_fwd_f32`` and the atomics-free, output-stationary ``csn_point_interp_bwd_f32``.  A field built from CPU tensors
forms the average with ``index_add_`` (a data-loader worker has no device); nothing on the device ever takes that path, and
``interpolate`` has no CPU path at all.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as CF
from .minkowski_conv import _B_BITS, _C_BIAS, _pack, _unpack, build_kernel_map
from .minkowski_csn import offsets_from_batch_index
from .minkowski_hrnet import VoxelPyramid, build_pyramid
from .minkowski_unet import UNetPyramid, build_unet_pyramid

_NO_CPU = "csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path"
QUANTIZATION_MODES = ("random_subsample", "unweighted_average")
MAX_INTERP_WIDTH = 1024
MAX_MEAN_WIDTH = 64


def _rows_ok(t: torch.Tensor, width: int) -> bool:
    return t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= width)


def voxel_mean(feats: torch.Tensor, vox_ptr: torch.Tensor, vox_pts: torch.Tensor) -> torch.Tensor:
    """``out (Nv, Cf)``: the mean of ``feats (Np, Cf)`` over the points of every voxel of the CSR, added in CSR order
    (``csn_voxel_mean_f32``)."""
    CF._need_cuda(feats, vox_ptr, vox_pts)
    if feats.dim() != 2 or not 1 <= feats.shape[1] <= MAX_MEAN_WIDTH:
        raise ValueError(f"feats must be (Np, Cf) with Cf in [1, {MAX_MEAN_WIDTH}]")
    if not _rows_ok(feats, feats.shape[1]):
        feats = feats.contiguous()
    n_pts, cf = feats.shape
    n_vox = vox_ptr.numel() - 1
    if vox_pts.numel() != n_pts or n_vox < 1:
        raise ValueError("the CSR does not fit the points")
    out = torch.empty((n_vox, cf), device=feats.device, dtype=torch.float32)
    _lib.check(_lib.lib().csn_voxel_mean_f32(CF._ptr(feats), feats.stride(0) if n_pts > 1 else cf, n_pts, CF._ptr(vox_ptr),
                                             CF._ptr(vox_pts), n_vox, cf, CF._ptr(out), cf, CF._stream()), "csn_voxel_mean_f32")
    return out


def _check_out(out: Optional[torch.Tensor], rows: int, width: int, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty((rows, width), device=like.device, dtype=torch.float32)
    CF._need_cuda(out)
    if out.dim() != 2 or tuple(out.shape) != (rows, width) or not _rows_ok(out, width) or out.device != like.device:
        raise ValueError(f"out must be ({rows}, {width}) rows with contiguous columns on the input's device")
    return out


def _pitch(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def interpolate_rows(z: torch.Tensor, coords: torch.Tensor, home: torch.Tensor, table: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y (Np, C)`` of ``csn_point_interp_fwd_f32`` — no autograd.  ``z (Nv, C)`` may be a column block of a wider buffer, and so
    may ``out``: its columns beyond C are left untouched."""
    CF._need_cuda(z, coords, home, table)
    n_vox, c = z.shape
    n_pts = coords.shape[0]
    if not _rows_ok(z, c):
        z = z.contiguous()
    y = _check_out(out, n_pts, c, z)
    _lib.check(_lib.lib().csn_point_interp_fwd_f32(CF._ptr(z), _pitch(z), n_vox, CF._ptr(coords), CF._ptr(home), CF._ptr(table), n_pts, c,
                                                   CF._ptr(y), _pitch(y), CF._stream()), "csn_point_interp_fwd_f32")
    return y


def interpolate_rows_backward(dy: torch.Tensor, coords: torch.Tensor, vox_ptr: torch.Tensor, vox_pts: torch.Tensor,
                              table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dz (Nv, C)`` of ``csn_point_interp_bwd_f32``: the adjoint of ``interpolate_rows`` applied to ``dy (Np, C)``."""
    CF._need_cuda(dy, coords, vox_ptr, vox_pts, table)
    n_pts, c = dy.shape
    n_vox = vox_ptr.numel() - 1
    if not _rows_ok(dy, c):
        dy = dy.contiguous()
    dz = _check_out(out, n_vox, c, dy)
    _lib.check(_lib.lib().csn_point_interp_bwd_f32(CF._ptr(dy), _pitch(dy), n_pts, CF._ptr(coords), CF._ptr(vox_ptr), CF._ptr(vox_pts),
                                                   CF._ptr(table), n_vox, c, CF._ptr(dz), _pitch(dz), CF._stream()),
               "csn_point_interp_bwd_f32")
    return dz


class _Interpolate(torch.autograd.Function):
    """y = interpolate(z) through ``csn_point_interp_fwd_f32`` / ``csn_point_interp_bwd_f32``; the field's arrays are constants."""

    @staticmethod
    def forward(ctx, z, field, table):
        ctx.field, ctx.table = field, table
        return interpolate_rows(z, field.coords, field.home, table)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        f = ctx.field
        return interpolate_rows_backward(dy, f.coords, f.vox_ptr, f.vox_pts, ctx.table), None, None


class PointField:
    """``ME.TensorField(feats, coords, quantization_mode=...)`` for the module docstring's semantics.

    Attributes (all on the device of ``coords``): ``coords (Np, 4)`` float32, ``feats (Np, Cf)`` float32, ``voxel_coords (Nv, 4)``
    int64 sorted by (b, x, y, z), ``home (Np,)`` int32 (MinkowskiEngine's inverse mapping), ``vox_ptr (Nv + 1,)`` / ``vox_pts (Np,)``
    int32 (the points of every voxel, ascending inside a voxel); ``offsets`` / ``voxel_offsets`` (B + 1,) int64 on the CPU: the
    point rows / voxel rows of every shape, for ``seg_loss``."""

    def __init__(self, coords: torch.Tensor, feats: torch.Tensor, quantization_mode: str = "random_subsample"):
        if quantization_mode not in QUANTIZATION_MODES:
            raise ValueError(f"quantization_mode must be one of {QUANTIZATION_MODES}")
        if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < 1 or coords.dtype != torch.float32:
            raise ValueError("coords must be a non-empty (Np, 4) float32 tensor [b, x, y, z] in voxel units")
        if feats.dim() != 2 or feats.shape[0] != coords.shape[0] or feats.shape[1] < 1 or feats.dtype != torch.float32:
            raise ValueError("feats must be (Np, Cf) float32, one row per point")
        if feats.device != coords.device:
            raise ValueError("coords and feats must be on one device")
        if not bool(torch.isfinite(coords).all()):
            raise ValueError("coords hold NaN or inf")
        b = coords[:, 0]
        if bool((b != b.floor()).any()) or bool((b < 0).any()) or bool((b >= (1 << _B_BITS)).any()):
            raise ValueError(f"batch indices must be integers in [0, {1 << _B_BITS})")
        if bool((b[1:] < b[:-1]).any()):
            raise ValueError("batch indices must be non-decreasing: the points are not sorted by shape")
        fl = coords[:, 1:].floor()
        if bool((fl < -_C_BIAS).any()) or bool((fl >= _C_BIAS).any()):
            raise ValueError(f"floor(x, y, z) must lie in [{-_C_BIAS}, {_C_BIAS})")
        self.quantization_mode = quantization_mode
        self.coords, self.feats = coords.contiguous(), feats.contiguous()
        keys = _pack(torch.cat([b.long()[:, None], fl.long()], dim=1))
        skeys, order = torch.sort(keys, stable=True)                # stable: ascending point numbers inside a voxel
        uniq, counts = torch.unique_consecutive(skeys, return_counts=True)
        n_vox = uniq.numel()
        self.voxel_coords = _unpack(uniq)
        self.vox_ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
        self.vox_pts = order.int()
        home = torch.empty_like(order)
        home[order] = torch.repeat_interleave(torch.arange(n_vox, device=coords.device), counts)
        self.home = home.int()
        self.offsets = offsets_from_batch_index(b)
        self.voxel_offsets = offsets_from_batch_index(self.voxel_coords[:, 0])
        self._voxel_feats: Optional[torch.Tensor] = None
        self._pyramid: Optional[VoxelPyramid] = None
        self._unet_pyramid: Optional[UNetPyramid] = None
        self._table: Optional[torch.Tensor] = None

    @classmethod
    def from_keys(cls, coords: torch.Tensor, feats: torch.Tensor, keys: torch.Tensor, status: torch.Tensor, offsets,
                  quantization_mode: str = "random_subsample") -> "PointField":
        """The field ``PointField(coords, feats, quantization_mode)`` builds — every attribute equal — from what a
        ``csn_amd.minkowski_points.PointBatch`` already knows: ``keys (Np,)`` int64 the packed key of every point's home voxel,
        ``status (1,)`` int32 the device word the batch kernels flagged bad points in, ``offsets (B + 1,)`` the point rows of every
        shape on the host.  One stable sort and one scan in torch, ONE host read (the status word, the voxel count and the voxel rows
        of every shape), then ``csn_field_index_i32`` (include/csn_hip.h section 18d) writes ``home``, ``vox_ptr``, ``vox_pts`` and
        the unique keys.  A non-zero status raises ``ValueError`` with the constructor's own message; device tensors only."""
        if quantization_mode not in QUANTIZATION_MODES:
            raise ValueError(f"quantization_mode must be one of {QUANTIZATION_MODES}")
        if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < 1 or coords.dtype != torch.float32:
            raise ValueError("coords must be a non-empty (Np, 4) float32 tensor [b, x, y, z] in voxel units")
        if feats.dim() != 2 or feats.shape[0] != coords.shape[0] or feats.shape[1] < 1 or feats.dtype != torch.float32:
            raise ValueError("feats must be (Np, Cf) float32, one row per point")
        n_pts = coords.shape[0]
        if keys.dim() != 1 or keys.shape[0] != n_pts or keys.dtype != torch.int64:
            raise ValueError("keys must be (Np,) int64, one packed key per point")
        if status.numel() != 1 or status.dtype != torch.int32:
            raise ValueError("status must be one int32 word")
        if len({coords.device, feats.device, keys.device, status.device}) != 1:
            raise ValueError("coords, feats, keys and status must be on one device")
        off = torch.as_tensor(offsets).reshape(-1).to("cpu", torch.int64)
        if off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != n_pts or bool((off[1:] <= off[:-1]).any()):
            raise ValueError("offsets must start at 0, increase strictly (every shape >= 1 point) and end at the point count")
        if off.numel() - 1 > (1 << _B_BITS):
            raise ValueError(f"batch indices must be integers in [0, {1 << _B_BITS})")
        if not coords.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        CF._need_cuda(coords, feats, status)
        dev = coords.device
        skeys, order = torch.sort(keys, stable=True)                # stable: ascending point numbers inside a voxel
        vid = torch.cat([skeys.new_zeros(1), (skeys[1:] != skeys[:-1]).cumsum(0)])
        starts = off[:-1].to(dev)
        word = torch.cat([status.reshape(1).long(), vid[-1:] + 1, vid[starts]]).tolist()       # the one host read
        if word[0] != 0:
            cls(coords, feats, quantization_mode)                   # the constructor's checks and message, the failing call's price
            raise ValueError(f"the points are not valid (point-batch status {word[0]})")
        n_vox = word[1]
        f = object.__new__(cls)
        f.quantization_mode = quantization_mode
        f.coords, f.feats = coords.contiguous(), feats.contiguous()
        f.home = torch.empty(n_pts, dtype=torch.int32, device=dev)
        f.vox_ptr = torch.empty(n_vox + 1, dtype=torch.int32, device=dev)
        f.vox_pts = torch.empty(n_pts, dtype=torch.int32, device=dev)
        uniq = torch.empty(n_vox, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)       # (raised only by arrays that are no sort and scan: not read)
        _lib.check(_lib.lib().csn_field_index_i32(CF._ptr(skeys), CF._ptr(order), CF._ptr(vid), n_pts, n_vox, CF._ptr(f.home),
                                                  CF._ptr(f.vox_ptr), CF._ptr(f.vox_pts), CF._ptr(uniq), CF._ptr(flags), CF._stream()),
                   "csn_field_index_i32")
        f.voxel_coords = _unpack(uniq)
        f.offsets = off
        f.voxel_offsets = torch.tensor(word[2:] + [n_vox], dtype=torch.int64)
        f._voxel_feats = f._pyramid = f._unet_pyramid = f._table = None
        return f

    # ---- sizes ----
    @property
    def n_points(self) -> int:
        return self.coords.shape[0]

    @property
    def n_voxels(self) -> int:
        return self.voxel_coords.shape[0]

    @property
    def device(self) -> torch.device:
        return self.coords.device

    # ---- the voxel side ----
    @property
    def voxel_feats(self) -> torch.Tensor:
        """(Nv, Cf): the features of the voxel rows under the field's quantisation mode."""
        if self._voxel_feats is None:
            first = self.vox_pts[self.vox_ptr[:-1].long()].long()
            if self.quantization_mode == "random_subsample":
                self._voxel_feats = self.feats.index_select(0, first)
            elif self.feats.is_cuda:
                if self.feats.shape[1] > MAX_MEAN_WIDTH:
                    raise ValueError(f"unweighted_average takes up to {MAX_MEAN_WIDTH} feature channels")
                self._voxel_feats = voxel_mean(self.feats, self.vox_ptr, self.vox_pts)
            else:                                                       # host-side preparation (module docstring)
                total = torch.zeros((self.n_voxels, self.feats.shape[1]), dtype=torch.float32)
                total.index_add_(0, self.home.long(), self.feats)
                self._voxel_feats = total / (self.vox_ptr[1:] - self.vox_ptr[:-1]).float()[:, None]
        return self._voxel_feats

    def pyramid(self, n_levels: int, stem_kernel: int = 5, backend: Optional[str] = None) -> VoxelPyramid:
        """The ``VoxelPyramid`` of ``voxel_coords``, built once and kept (a different request rebuilds it).  ``backend`` as in
        ``build_pyramid`` (both give the same pyramid, so it is no part of the request)."""
        p = self._pyramid
        if p is None or p.n_levels != n_levels or p.stem_kernel != stem_kernel:
            self._pyramid = p = build_pyramid(self.voxel_coords, n_levels, stem_kernel, backend=backend)
            self._table = p.s1[0].fwd
        return p

    def unet_pyramid(self, stem_kernel: int = 5, backend: Optional[str] = None) -> UNetPyramid:
        """The ``UNetPyramid`` of ``voxel_coords`` for a ``Res16UNet*`` — ``model((field.unet_pyramid(), field.voxel_feats))`` —, built
        once and kept like ``pyramid()`` (a different stem kernel rebuilds it).  ``backend`` as in ``build_unet_pyramid`` (both give
        the same pyramid, so it is no part of the request).  Its level-0 kernel-3 map serves ``corner_table`` where none is there."""
        p = self._unet_pyramid
        if p is None or p.stem_kernel != stem_kernel:
            self._unet_pyramid = p = build_unet_pyramid(self.voxel_coords, stem_kernel, backend=backend)
            if self._table is None:
                self._table = p.s1[0].fwd
        return p

    def sparse(self) -> Tuple[object, torch.Tensor]:
        """``field.sparse()``: ``(pyramid or voxel_coords, voxel_feats)`` — a batch that ``HRNetSimCSN.forward`` / ``backbone_rows``
        take as it stands (the pyramid once ``pyramid()`` was called, the coordinates otherwise)."""
        return (self._pyramid if self._pyramid is not None else self.voxel_coords), self.voxel_feats

    def corner_table(self, backend: Optional[str] = None) -> torch.Tensor:
        """(27, Nv) int32: the kernel-3 stride-1 map of the voxel rows — the pyramid's if one was built, else built once here
        (``backend`` as in ``build_kernel_map``)."""
        if self._table is None:
            self._table = build_kernel_map(self.voxel_coords, kernel_size=3, stride=1, tensor_stride=1, backend=backend).fwd
        return self._table

    # ---- the point side ----
    def interpolate(self, z: torch.Tensor) -> torch.Tensor:
        """``soutput.interpolate(field)``: ``y (Np, C)`` of a map ``z (Nv, C)`` on the field's voxel rows, C in [1, 1024], with the
        adjoint as its gradient (one autograd node)."""
        if z.dim() != 2 or z.shape[0] != self.n_voxels:
            raise ValueError(f"z must be (Nv, C) on the field's {self.n_voxels} voxel rows")
        if not 1 <= z.shape[1] <= MAX_INTERP_WIDTH:
            raise ValueError(f"width {z.shape[1]} is not supported: 1 to {MAX_INTERP_WIDTH}")
        if not (z.is_cuda and self.coords.is_cuda):
            raise _lib.CsnError(_NO_CPU)
        CF._need_cuda(z)
        if z.device != self.device:
            raise ValueError("z and the field must be on one device")
        return _Interpolate.apply(z, self, self.corner_table())

    def to(self, device) -> "PointField":
        """The field on ``device``: every array moves, nothing is rebuilt."""
        f = object.__new__(PointField)
        f.quantization_mode = self.quantization_mode
        for name in ("coords", "feats", "voxel_coords", "vox_ptr", "vox_pts", "home"):
            setattr(f, name, getattr(self, name).to(device))
        f.offsets, f.voxel_offsets = self.offsets, self.voxel_offsets
        f._voxel_feats = None if self._voxel_feats is None else self._voxel_feats.to(device)
        f._pyramid = None if self._pyramid is None else self._pyramid.to(device)
        f._unet_pyramid = None if self._unet_pyramid is None else self._unet_pyramid.to(device)
        f._table = f._pyramid.s1[0].fwd if f._pyramid is not None else (None if self._table is None else self._table.to(device))
        return f


def batch_points(shapes: Sequence[Sequence[torch.Tensor]], voxel_size: float):
    """``Voxelizer.voxelize`` + ``cfl_collate_fn`` for ``PointField``: ``shapes`` is a list of ``(xyz (n, 3), feats (n, Cf))`` or
    ``(xyz, feats, labels (n,))``.  The coordinates are divided by ``voxel_size`` in float64 and cast to float32, the batch column is
    prepended and the shapes are concatenated.  Returns ``(coords (Np, 4) float32, feats (Np, Cf) float32)`` — and the concatenated
    labels (int64) when every shape brings them."""
    if len(shapes) < 1 or not voxel_size > 0:
        raise ValueError("batch_points needs at least one shape and a positive voxel size")
    coords, feats, labels = [], [], []
    for i, shape in enumerate(shapes):
        xyz, f = torch.as_tensor(shape[0]), torch.as_tensor(shape[1])
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or f.dim() != 2 or f.shape[0] != xyz.shape[0]:
            raise ValueError("every shape is (xyz (n, 3), feats (n, Cf)[, labels (n,)]) with n >= 1")
        v = (xyz.double() / float(voxel_size)).float()
        coords.append(torch.cat([torch.full((v.shape[0], 1), float(i), dtype=torch.float32, device=v.device), v], dim=1))
        feats.append(f.float())
        if len(shape) > 2:
            labels.append(torch.as_tensor(shape[2]).reshape(-1).long())
    if labels and len(labels) != len(shapes):
        raise ValueError("either every shape brings labels or none does")
    out = (torch.cat(coords), torch.cat(feats))
    return out + (torch.cat(labels),) if labels else out
