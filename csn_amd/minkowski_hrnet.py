"""MinkowskiNet's HRNet backbone and ``HRNetSimCSN`` on voxel rows, on the MI355X kernels.

Reference (marios2019/CSN):
  * ``HRNetBase.backbone_initialization`` / ``forward_backbone``        MinkowskiNet/models/hrnet.py:31-163
  * final transitions, the concatenation, ``fc_layer``, the head        MinkowskiNet/models/hrnet.py:308-357, 425-454
  * ``BasicBlock``                                                      MinkowskiNet/models/modules/resnet_block.py:22-57

Every convolution of the backbone is followed by a BatchNorm, and every BatchNorm by a ReLU, a residual add or a sum over branches.
With ``fused=True`` each such pair is two autograd nodes on include/csn_hip.h section 15:

  * ``conv_stats``  (15a) the gather-GEMM with the BatchNorm statistics formed in its epilogue: z, mean, invstd, running statistics;
  * ``bn_act``      (15b) y = act(sum_m (gamma_m (z_m - mean_m) s_m + beta_m) + r) for up to three terms, whose backward is the
                    COMPLETE BatchNorm gradient of every term (the statistics are constants of the autograd graph, as in
                    ``_RowsFC``).
In eval mode the convolution is the plain ``sparse_conv3d`` and ``bn_act`` takes the running statistics.  With ``fused=False`` the same
graph runs on ``sparse_conv3d`` + ``F.batch_norm`` + ATen add / ReLU: the timing baseline and the error yardstick of the tests.

The three or four maps that the reference joins with ``me.cat`` are joined with ``torch.cat`` here.

Inference (``tuning.override(eval_epilogue=True)``, a fused backbone in eval mode with autograd disabled): every convolution + norm is
ONE launch of include/csn_hip.h section 19 (``sparse_conv_bn_act``: the BatchNorm on its running statistics, the residual and the
ReLU in the product's epilogue), a branch sum is a chain of such launches into one buffer, and the concatenated result is
allocated once and written in place through the kernels' output pitch: no ``torch.cat``.  Off by default.
With ``infer_maps16`` on top, in math mode "bf16" / "fp16" with ``rows_single_product``, the maps between those launches are bf16 /
fp16 rows (section 24, ``sparse_conv_bn_act`` on 16-bit tensors); the stem's input and the result stay fp32.  Off by default.

Training on bf16 maps (``tuning.override(train_maps16=True)``, a fused backbone in training mode on a plain ``VoxelPyramid``, math mode
"bf16" with ``rows_single_product``): every ReLU output that only these nodes read is stored as bf16 rows — a ``Map16`` — and gathered
as it lies by the next convolution and its weight gradient (include/csn_hip.h section 28); z, the statistics, the gradient maps and
the maps ``torch.cat`` joins stay fp32.  Off by default; ignored everywhere else.

Grouped passes (include/csn_hip.h section 20): the K + 1 batches of a CSN training step merged into ONE coordinate set with
shifted batch indices (``merge_batches`` -> ``GroupedPyramid``).  The rows of a batch are then a contiguous range at every level, the
convolutions run once on the merged maps, and ``conv_stats_groups`` / ``bn_act_groups`` take the BatchNorm statistics per row group.
``tuning.override(grouped_passes=True)`` makes ``HRNetSimCSN.forward`` do so.  Off by default.

``VoxelPyramid`` holds the coordinate sets and kernel maps of one batch, built once (``build_pyramid``): level l's coordinates are
``down^l(coords)`` by the stride-2 rule of ``build_kernel_map``; per level the stride-1 kernel-3 map, at level 0 the stem's map,
between neighbouring levels the stride-2 map whose ``transpose()`` serves the up direction.

Offset numbering and the sorted order of the coarse levels are this project's choice (minkowski_conv.py): parity unpinned against
MinkowskiEngine's own checkpoints.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as CF
from . import minkowski_conv as _mc
from . import tuning
from .minkowski_conv import KernelMap, SparseConv3d, SparseConvTranspose3d, build_kernel_map, sparse_conv3d
from .minkowski_csn import BackboneFC, SimCSNHead, offsets_from_batch_index

_NO_CPU = "csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path"


# ------------------------------------------------------------------------------------------------------
# the pyramid
# ------------------------------------------------------------------------------------------------------
class VoxelPyramid:
    """Coordinates and kernel maps of one batch for an ``n_levels``-branch HRNet.

    ``coords[l]`` (n_l, 4) at tensor stride 2^l; ``s1[l]`` the kernel-3 stride-1 map of level l; ``stem`` the kernel-``stem_kernel``
    stride-1 map of level 0; ``down[l]`` the kernel-3 stride-2 map from level l onto level l + 1; ``up(l)`` its transpose (from level
    l + 1 onto level l)."""

    def __init__(self, coords: List[torch.Tensor], s1: List[KernelMap], stem: KernelMap, down: List[KernelMap], stem_kernel: int):
        self.coords, self.s1, self.stem, self.down, self.stem_kernel = coords, s1, stem, down, stem_kernel
        self._up = [d.transpose() for d in down]

    @property
    def n_levels(self) -> int:
        return len(self.coords)

    def up(self, level: int) -> KernelMap:
        return self._up[level]

    def to(self, device) -> "VoxelPyramid":
        return VoxelPyramid([c.to(device) for c in self.coords], [m.to(device) for m in self.s1], self.stem.to(device),
                            [m.to(device) for m in self.down], self.stem_kernel)


def build_pyramid(coords: torch.Tensor, n_levels: int, stem_kernel: int = 5, backend: Optional[str] = None) -> VoxelPyramid:
    """The pyramid of ``coords`` (n, 4) = [b, x, y, z] at tensor stride 1 (device or CPU tensor; the maps live where it does).
    ``backend`` as in ``build_kernel_map``: ``"torch"``, ``"hip"`` (device tensors only) or None for the tuning switch
    ``native_kernel_maps``; both give the same pyramid."""
    if n_levels < 1:
        raise ValueError("n_levels must be at least 1")
    backend = _mc.resolve_backend(backend, coords)
    if backend == "hip":
        return _build_pyramid_hip(coords, n_levels, stem_kernel)
    levels, s1, down = [coords.long()], [], []
    for l in range(n_levels):
        ts = 1 << l
        s1.append(build_kernel_map(levels[l], kernel_size=3, stride=1, tensor_stride=ts, backend=backend))
        if l + 1 < n_levels:
            d = build_kernel_map(levels[l], kernel_size=3, stride=2, tensor_stride=ts, backend=backend)
            down.append(d)
            levels.append(d.out_coords)
    stem = s1[0] if stem_kernel == 3 else build_kernel_map(levels[0], kernel_size=stem_kernel, stride=1, tensor_stride=1,
                                                           backend=backend)
    return VoxelPyramid(levels, s1, stem, down, stem_kernel)


def _build_pyramid_hip(coords: torch.Tensor, n_levels: int, stem_kernel: int) -> VoxelPyramid:
    """The same pyramid on include/csn_hip.h section 17.  Level l's keys and their sort are formed once and serve ``s1[l]``, the stem
    and ``down[l]``; a coarser level leaves ``torch.unique`` sorted, so it is never sorted again.  Level 0 takes one key launch; a
    coarser level takes one launch for the floored keys and one key launch on its unpacked coordinates, which computes nothing new
    (its keys equal the unique ones) and is there as the level's range and tensor-stride check, the torch backend's
    ``_check_coords`` of that level; one lookup launch per table; one status word for the whole pyramid, read once at the end."""
    if stem_kernel < 1 or stem_kernel % 2 == 0:
        raise ValueError(f"kernel_size {stem_kernel} is not supported: odd sizes only")
    if stem_kernel not in (1, 3, 5):
        raise ValueError(f"kernel_size {stem_kernel} is not supported: the kernels take 1, 3 and 5")
    status = _mc._new_status(coords.device)
    sets, s1, down = [_mc._key_set(coords, 1, "coords", status)], [], []
    for l in range(n_levels):
        ts, here = 1 << l, sets[l]
        fwd = _mc._lookup(here, here, 3, ts, status)
        s1.append(KernelMap(here.coords, here.coords, 3, 1, ts, ts, False, fwd, None))
        if l + 1 < n_levels:
            up = _mc._coarse_set(here, 2 * ts)
            up.keys = _mc._coord_keys(up.coords, 2 * ts, status)
            sets.append(up)
            down.append(KernelMap(here.coords, up.coords, 3, 2, ts, 2 * ts, False, _mc._lookup(here, up, 3, ts, status),
                                  _mc._lookup(up, here, 3, -ts, status)))
    if stem_kernel == 3:
        stem = s1[0]
    else:
        stem = KernelMap(sets[0].coords, sets[0].coords, stem_kernel, 1, 1, 1, False,
                         _mc._lookup(sets[0], sets[0], stem_kernel, 1, status), None)
    _mc._raise_for_status(_mc._read_status(status), [(coords, 1, "coords")])
    return VoxelPyramid([s.coords for s in sets], s1, stem, down, stem_kernel)


MAX_GROUPS = 8                                        # the head's own limit: K + 1 <= 8


class GroupedPyramid:
    """The ``VoxelPyramid`` of G batches merged into one coordinate set (``merge_batches`` / ``group_pyramid``), and where every
    batch's rows lie in it.  The batch index leads the sort, so group g's rows are one contiguous range at EVERY level: the same
    rows in the same order as in that batch's own pyramid.

    ``pyramid`` the ``VoxelPyramid``; ``group_rows[l]`` (G + 1,) int32 on the pyramid's device: the row offsets of the groups at
    level l; ``group_rows_host[l]`` the same numbers as a list; ``n_shapes[g]`` the shapes of group g and ``shape_offsets`` (G + 1)
    their running sum: group g's shapes carry the batch indices ``[shape_offsets[g], shape_offsets[g + 1])``; ``row_offsets``
    (total shapes + 1, a host list) the level-0 row offset of every shape.  ``coords``, ``s1``, ``stem``, ``down``, ``up``,
    ``n_levels`` and ``stem_kernel`` are the pyramid's."""

    def __init__(self, pyramid: VoxelPyramid, group_rows: List[torch.Tensor], group_rows_host: List[List[int]], n_shapes: List[int],
                 row_offsets: Optional[List[int]]):
        self.pyramid, self.group_rows, self.group_rows_host, self.n_shapes = pyramid, group_rows, group_rows_host, list(n_shapes)
        self.shape_offsets = [0]
        for n in self.n_shapes:
            self.shape_offsets.append(self.shape_offsets[-1] + n)
        self._row_offsets = row_offsets

    coords = property(lambda self: self.pyramid.coords)
    s1 = property(lambda self: self.pyramid.s1)
    stem = property(lambda self: self.pyramid.stem)
    down = property(lambda self: self.pyramid.down)
    stem_kernel = property(lambda self: self.pyramid.stem_kernel)
    n_levels = property(lambda self: self.pyramid.n_levels)

    def up(self, level: int) -> KernelMap:
        return self.pyramid.up(level)

    @property
    def n_groups(self) -> int:
        return len(self.n_shapes)

    @property
    def row_offsets(self) -> List[int]:
        """Level-0 row offset of every shape (a host list).  Known from the construction's one host read when ``n_shapes`` was
        given or the coordinates were host tensors; otherwise read here, once."""
        if self._row_offsets is None:
            self._row_offsets = [int(v) for v in offsets_from_batch_index(self.coords[0][:, 0], self.shape_offsets[-1]).tolist()]
        return self._row_offsets

    def group_offsets(self, g: int) -> List[int]:
        """The (n_shapes[g] + 1) row offsets of group g's shapes inside the group's own level-0 rows: what the head takes."""
        ro = self.row_offsets
        a, b = self.shape_offsets[g], self.shape_offsets[g + 1]
        return [v - ro[a] for v in ro[a:b + 1]]

    def groups(self, level: int) -> Tuple[torch.Tensor, int]:
        return self.group_rows[level], self.n_groups

    def to(self, device) -> "GroupedPyramid":
        return GroupedPyramid(self.pyramid.to(device), [t.to(device) for t in self.group_rows], self.group_rows_host, self.n_shapes,
                              self._row_offsets)


def group_pyramid(coords: torch.Tensor, n_shapes: Sequence[int], n_levels: int, stem_kernel: int = 5,
                  backend: Optional[str] = None) -> GroupedPyramid:
    """The ``GroupedPyramid`` of ``coords (n, 4)`` that ALREADY hold G batches one after the other with running batch indices
    (group g's shapes are ``[sum n_shapes[:g], sum n_shapes[:g + 1])``; rows sorted by shape).  The pyramid is ``build_pyramid``'s;
    on top of what that does, ONE host read: every level's group row offsets (and the level-0 row offset of every shape) in one
    transfer.  It is checked there that the offsets start at 0, ascend and end at the level's row count — no kernel is launched on
    offsets nobody looked at — and a group with exactly one row at any level raises ``ValueError``."""
    n_shapes = [int(v) for v in n_shapes]
    if not 1 <= len(n_shapes) <= MAX_GROUPS:
        raise ValueError(f"1 to {MAX_GROUPS} groups (K + 1 <= {MAX_GROUPS}), not {len(n_shapes)}")
    if min(n_shapes) < 1:
        raise ValueError("every group needs at least one shape")
    pyr = build_pyramid(coords, n_levels, stem_kernel, backend=backend)
    dev = pyr.coords[0].device
    total = sum(n_shapes)
    bounds = torch.tensor([sum(n_shapes[:g]) for g in range(len(n_shapes) + 1)], dtype=torch.int64, device=dev)
    found = [torch.searchsorted(c[:, 0].contiguous(), bounds) for c in pyr.coords]
    b0 = pyr.coords[0][:, 0].contiguous()
    found.append(torch.searchsorted(b0, torch.arange(total + 1, dtype=torch.int64, device=dev)))
    found.append((b0[1:] < b0[:-1]).any().long().reshape(1))
    host = torch.cat(found).tolist()                                        # the one host read
    if host.pop():
        raise ValueError("batch-index column is not non-decreasing: the rows are not sorted by shape")
    G1 = len(n_shapes) + 1
    rows_host = [host[l * G1:(l + 1) * G1] for l in range(n_levels)]
    row_offsets = host[n_levels * G1:]
    group_rows = _level_rows(pyr, rows_host, True)
    if any(b <= a for a, b in zip(row_offsets, row_offsets[1:])):
        raise ValueError("every shape of the batch needs at least one row")
    return GroupedPyramid(pyr, group_rows, rows_host, n_shapes, row_offsets)


def _level_rows(pyr: VoxelPyramid, rows_host: List[List[int]], given: bool) -> List[torch.Tensor]:
    """Checks every level's group row offsets as the host read them (they start at 0, ascend, end at the level's row count; no group
    has one row or none) and returns them as int32 tensors on the pyramid's device.  ``given``: the caller stated the groups' shape
    counts, so offsets out of order mean batch indices that do not fit them, and an empty group is told apart."""
    for l, off in enumerate(rows_host):
        n_l, steps = pyr.coords[l].shape[0], list(zip(off, off[1:]))
        if off[0] != 0 or off[-1] != n_l or any(b < a or (b == a and not given) for a, b in steps):
            raise ValueError(f"level {l}: the group row offsets {off} do not start at 0, ascend and end at the {n_l} rows"
                             + (": the batch indices are not sorted, or leave the groups' shapes" if given else ""))
        if any(b == a for a, b in steps):
            raise ValueError(f"level {l}: a group has no rows")
        if any(b - a == 1 for a, b in steps):
            raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance): "
                             f"a group has exactly one row at level {l}")
    dev = pyr.coords[0].device
    return [torch.tensor(off, dtype=torch.int32).to(dev) for off in rows_host]


def merge_batches(batches: Sequence, n_levels: int, stem_kernel: int = 5, n_shapes: Optional[Sequence[int]] = None,
                  backend: Optional[str] = None) -> GroupedPyramid:
    """G batches ``(coords (n_g, 4), feats)``, 1 <= G <= 8, as ONE coordinate set: group g's batch column is shifted by the number of
    shapes in groups 0 .. g - 1 (``n_shapes[g]`` where given — a ``PointBatch`` knows it on the host —, else the group's largest batch
    index + 1) and the coordinates are concatenated, which keeps them sorted.  The pyramid is ``build_pyramid``'s with either
    backend; shifted batch indices that leave the range it accepts raise as it does.  Beyond ``build_pyramid``'s own, the
    construction does one host read (``group_pyramid``); without ``n_shapes`` on device tensors the shape counts are that read
    and the per-shape row offsets a second one, taken when ``row_offsets`` is first asked for.  The features are the caller's to
    concatenate (``torch.cat([f for _, f in batches])``)."""
    if not 1 <= len(batches) <= MAX_GROUPS:
        raise ValueError(f"1 to {MAX_GROUPS} batches (K + 1 <= {MAX_GROUPS}), not {len(batches)}")
    cs = [b[0] for b in batches]
    for c in cs:
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 4 or c.shape[0] < 1:
            raise ValueError("every batch needs (n, 4) coordinates [b, x, y, z] with n >= 1")
    if n_shapes is not None:
        n_shapes = [int(v) for v in n_shapes]
        if len(n_shapes) != len(cs):
            raise ValueError("n_shapes needs one entry per batch")
    elif not cs[0].is_cuda:
        n_shapes = [int(c[:, 0].max()) + 1 for c in cs]
    if n_shapes is not None:
        shifted = [c.long() if g == 0 else c.long() + c.new_tensor([sum(n_shapes[:g]), 0, 0, 0], dtype=torch.int64)
                   for g, c in enumerate(cs)]
        return group_pyramid(torch.cat(shifted), n_shapes, n_levels, stem_kernel, backend)
    # device tensors, shape counts unknown: shift on the device, and learn the counts in the one read
    counts = torch.stack([c[:, 0].max().long() + 1 for c in cs])
    shifts = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    e0 = torch.tensor([1, 0, 0, 0], dtype=torch.int64, device=cs[0].device)
    merged = torch.cat([c.long() + shifts[g] * e0 for g, c in enumerate(cs)])
    pyr = build_pyramid(merged, n_levels, stem_kernel, backend=backend)
    found = [torch.searchsorted(c[:, 0].contiguous(), shifts) for c in pyr.coords]
    b0 = pyr.coords[0][:, 0].contiguous()
    host = torch.cat([counts] + found + [(b0[1:] < b0[:-1]).any().long().reshape(1)]).tolist()      # the one host read
    if host.pop():
        raise ValueError("batch-index column is not non-decreasing: the rows are not sorted by shape")
    G = len(cs)
    n_shapes, rows_host = host[:G], [host[G + l * (G + 1):G + (l + 1) * (G + 1)] for l in range(n_levels)]
    return GroupedPyramid(pyr, _level_rows(pyr, rows_host, False), rows_host, n_shapes, None)


# ------------------------------------------------------------------------------------------------------
# autograd nodes on sections 15 (the whole map is one BatchNorm batch) and 20 (``group_rows``: a batch per row group)
# ------------------------------------------------------------------------------------------------------
def _check_groups(group_rows: torch.Tensor, like: torch.Tensor) -> int:
    if not isinstance(group_rows, torch.Tensor) or group_rows.dtype != torch.int32 or group_rows.dim() != 1:
        raise ValueError("group_rows must be a (G + 1,) int32 tensor of row offsets")
    G = group_rows.numel() - 1
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"1 to {MAX_GROUPS} groups, not {G}")
    if not group_rows.is_cuda or group_rows.device != like.device:
        raise _lib.CsnError(_NO_CPU)
    return G


class _ConvStats(torch.autograd.Function):
    """(z, mean, invstd) = ``csn_sparse_conv_stats_fwd_f32``, or with ``group_rows`` ``csn_sparse_conv_stats_groups_fwd_f32``: mean /
    invstd are then (G, c_out) and the running statistics take G updates in group order; updates the running statistics in place.
    mean / invstd are constants of the graph; the backward is ``csn_sparse_conv_bwd_f32`` (on the merged map)."""

    @staticmethod
    def forward(ctx, x, w, kmap, group_rows, running_mean, running_var, eps, momentum):
        CF._need_cuda(x, w, kmap.fwd, running_mean, running_var)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        ctx.rows16 = tuning.current().rows_single_product
        x = x.contiguous()
        w_c = w.detach().contiguous()
        KV, c_in, c_out = w_c.shape
        n_in, n_out = kmap.n_in, kmap.n_out
        G = None
        if group_rows is not None:
            group_rows = group_rows.contiguous()
            G = group_rows.numel() - 1
        ws_n = int(L.csn_sparse_conv_stats_workspace_bytes(n_out, c_out) if group_rows is None else
                   L.csn_sparse_conv_stats_groups_workspace_bytes(n_out, c_out, G))
        z, mean, invstd, ws = _stats_outputs(n_out, c_out, ws_n, x.device, G)
        head = (CF._ptr(x), c_in, n_in, CF._ptr(kmap.fwd), n_out, KV, c_in, c_out, CF._ptr(w_c), CF._ptr(z), c_out, CF._ptr(mean),
                CF._ptr(invstd), CF._ptr(running_mean), CF._ptr(running_var), float(eps), float(momentum))
        with CF.rows16(ctx.rows16):
            if group_rows is None:
                _lib.check(L.csn_sparse_conv_stats_fwd_f32(*head, CF._ptr(ws), ws_n, CF._stream()), "csn_sparse_conv_stats_fwd_f32")
            else:
                _lib.check(L.csn_sparse_conv_stats_groups_fwd_f32(*head, group_rows.data_ptr(), G, CF._ptr(ws), ws_n, CF._stream()),
                           "csn_sparse_conv_stats_groups_fwd_f32")
        ctx.save_for_backward(x, w_c)
        ctx.kmap = kmap
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dmean, _dinvstd):
        with CF.math_mode(CF.backward_mode(ctx.mode)), CF.rows16(ctx.rows16):
            x, w = ctx.saved_tensors
            dx, dw, _ = _mc._sparse_conv_backward(dz, x, x.shape[1], w, ctx.kmap, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (dx, dw) + (None,) * 6


def _stats_outputs(n_out: int, c_out: int, ws_n: int, device, n_groups: Optional[int] = None):
    """``z``, ``mean``, ``invstd`` and the workspace of a convolution with the statistics epilogue (sections 15, 20, 26 - 28): one
    BatchNorm batch, or with ``n_groups`` one per row group and (G, c_out) statistics.  ``ws_n``: the entry point's byte count."""
    stats = (c_out,) if n_groups is None else (n_groups, c_out)
    z = torch.empty((n_out, c_out), device=device, dtype=torch.float32)
    mean = torch.empty(stats, device=device, dtype=torch.float32)
    invstd = torch.empty(stats, device=device, dtype=torch.float32)
    return z, mean, invstd, _mc._workspace(ws_n, device)


def _conv_stats(x, weight, kmap, grouped: bool, group_rows, running_mean, running_var, eps, momentum):
    if not (x.is_cuda and weight.is_cuda):
        raise _lib.CsnError(_NO_CPU)
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1] or weight.shape[0] != kmap.KV or x.shape[0] != kmap.n_in:
        raise ValueError("x must be (n_in, c_in) and weight (KV, c_in, c_out) for the map's KV and n_in")
    c_in, c_out = weight.shape[1], weight.shape[2]
    if c_out % 32 or not 32 <= c_out <= 256 or c_in > 256:
        raise ValueError("widths: c_out a multiple of 32 in [32, 256], c_in at most 256")
    G = _check_groups(group_rows, x) if grouped else None
    if kmap.n_out == 1 if G is None else kmap.n_out < 2 * G:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    pad = -c_in % 32
    if pad:
        x = F.pad(x, (0, pad))
        weight = F.pad(weight, (0, 0, 0, pad))
    return _ConvStats.apply(x.float(), weight, kmap, group_rows if grouped else None, running_mean, running_var, eps, momentum)


def conv_stats(x: torch.Tensor, weight: torch.Tensor, kmap: KernelMap, running_mean: Optional[torch.Tensor],
               running_var: Optional[torch.Tensor], eps: float, momentum: float):
    """``z (n_out, c_out)``, ``mean``, ``invstd`` of the convolution ``kmap`` describes and of its output's BatchNorm batch; the
    running statistics (either may be None) are updated in place.  An input width that is no multiple of 32 is zero-padded as in
    ``sparse_conv3d``.  A one-row output raises ``ValueError`` (no variance), as torch does.

    ``x`` may be a ``Map16`` (math mode "bf16" with ``tuning.rows_single_product``, else ``ValueError``): its bf16 rows are gathered as
    they lie, by the product and by its weight gradient (section 28) — z, mean and invstd are the bits of the call on the same
    values as fp32 —, and the backward's fp32 dx goes to the map's edge."""
    if isinstance(x, Map16):
        return _conv_stats16(x, weight, kmap, running_mean, running_var, eps, momentum)
    return _conv_stats(x, weight, kmap, False, None, running_mean, running_var, eps, momentum)


def conv_stats_groups(x: torch.Tensor, weight: torch.Tensor, kmap: KernelMap, group_rows: torch.Tensor,
                      running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], eps: float, momentum: float):
    """``conv_stats`` on a merged map whose output rows are G BatchNorm batches: ``group_rows (G + 1,)`` int32 on the device are the
    row offsets of the groups (``GroupedPyramid.group_rows[level]``: start at 0, ascend, end at ``kmap.n_out``, every group two rows
    or more — the CALLER has checked that, the kernels cannot).  Returns ``z (n_out, c_out)`` — the bits of ``conv_stats`` —,
    ``mean (G, c_out)`` and ``invstd (G, c_out)``; the running statistics (either may be None) take G updates in group order.
    Row groups have no bf16-map form: a ``Map16`` raises ``ValueError``."""
    if isinstance(x, Map16):
        raise ValueError("row groups have no bf16-map form (include/csn_hip.h section 28 takes the whole map as one batch)")
    return _conv_stats(x, weight, kmap, True, group_rows, running_mean, running_var, eps, momentum)


def _bn_unpack(flat, training):
    """The flat (z, mean, scale, gamma, beta) per term of a BatchNorm node as lists ``zs, means, scales, gammas, betas``, contiguous;
    in eval mode mean and scale are cloned: the running statistics may move before the backward."""
    M = len(flat) // 5
    zs = [flat[5 * m].contiguous() for m in range(M)]
    means = [flat[5 * m + 1].detach().contiguous() for m in range(M)]
    scales = [flat[5 * m + 2].detach().contiguous() for m in range(M)]
    if not training:
        means, scales = [t.clone() for t in means], [t.clone() for t in scales]
    gammas = [flat[5 * m + 3].detach().contiguous() for m in range(M)]
    betas = [flat[5 * m + 4].detach().contiguous() for m in range(M)]
    return zs, means, scales, gammas, betas


def _bn_terms(zs, means, scales, gammas, betas=None, grads=None) -> "_lib.BnTerms":
    """``CsnBnTerms`` of contiguous (N, C) terms: with ``betas`` for the forward, with ``grads`` = [(dz, dgamma, dbeta)] for the
    backward."""
    C = zs[0].shape[1]
    t = _lib.BnTerms()
    for m in range(len(zs)):
        t.z[m], t.ld_z[m], t.mean[m], t.scale[m], t.gamma[m] = CF._ptr(zs[m]), C, CF._ptr(means[m]), CF._ptr(scales[m]), CF._ptr(gammas[m])
        if betas is not None:
            t.beta[m] = CF._ptr(betas[m])
        if grads is not None:
            t.dz[m], t.ld_dz[m], t.dgamma[m], t.dbeta[m] = CF._ptr(grads[m][0]), C, CF._ptr(grads[m][1]), CF._ptr(grads[m][2])
    return t


def _bn_grads(need, at: int, M: int, N: int, C: int, dev):
    """[(dz, dgamma, dbeta)] per term, each None unless ``need`` (``needs_input_grad``, the terms from position ``at``) wants it, and
    the same as the tail of the node's return tuple."""
    grads, outs = [], []
    for m in range(M):
        nz, ng, nb = need[at + 5 * m], need[at + 5 * m + 3], need[at + 5 * m + 4]
        dz = torch.empty((N, C), device=dev, dtype=torch.float32) if nz else None
        dg = torch.empty((C,), device=dev, dtype=torch.float32) if ng else None
        db = torch.empty((C,), device=dev, dtype=torch.float32) if nb else None
        grads.append((dz, dg, db))
        outs += [dz, None, None, dg, db]
    return grads, outs


class _BnAct(torch.autograd.Function):
    """y = act(sum_m (gamma_m (z_m - mean_m) s_m + beta_m) + r) through ``csn_rows_bn_act_fwd_f32`` / ``_bwd_f32``, or with
    ``group_rows`` (training mode, (G, C) statistics per term) through ``csn_rows_bn_act_groups_fwd_f32`` / ``_bwd_f32``.
    Arguments after the fixed ones: (z, mean, scale, gamma, beta) per term."""

    @staticmethod
    def forward(ctx, relu, training, eps, group_rows, r, *flat):
        M = len(flat) // 5
        CF._need_cuda(r, *flat)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        zs, means, scales, gammas, betas = _bn_unpack(flat, training)
        N, C = zs[0].shape
        r_c = None if r is None else r.contiguous()
        y = torch.empty((N, C), device=zs[0].device, dtype=torch.float32)
        t = _bn_terms(zs, means, scales, gammas, betas=betas)
        tail = (CF._ptr(r_c), C, int(relu), CF._ptr(y), C, CF._stream())
        if group_rows is None:
            _lib.check(L.csn_rows_bn_act_fwd_f32(ctypes.addressof(t), M, N, C, int(training), float(eps), *tail), "csn_rows_bn_act_fwd_f32")
        else:
            group_rows = group_rows.contiguous()
            _lib.check(L.csn_rows_bn_act_groups_fwd_f32(ctypes.addressof(t), M, N, C, group_rows.data_ptr(), group_rows.numel() - 1, *tail),
                       "csn_rows_bn_act_groups_fwd_f32")
        ctx.save_for_backward(y if relu else None, group_rows, *zs, *means, *scales, *gammas)
        ctx.M, ctx.relu, ctx.training, ctx.eps, ctx.has_r = M, bool(relu), bool(training), float(eps), r is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        M = ctx.M
        saved = ctx.saved_tensors
        y, group_rows = saved[0], saved[1]
        zs, means, scales, gammas = (saved[2 + k * M:2 + (k + 1) * M] for k in range(4))
        L = _lib.lib()
        N, C = zs[0].shape
        dev = dy.device
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dr = torch.empty((N, C), device=dev, dtype=torch.float32) if (ctx.has_r and need[4]) else None
        grads, outs = _bn_grads(need, 5, M, N, C, dev)
        t = _bn_terms(zs, means, scales, gammas, grads=grads)
        head = (CF._ptr(dy), C, CF._ptr(y), C, ctypes.addressof(t), M, N, C)
        if group_rows is None:
            ws_n = int(L.csn_rows_bn_act_workspace_bytes(N, C, M))
            ws = _mc._workspace(ws_n, dev)
            _lib.check(L.csn_rows_bn_act_bwd_f32(*head, int(ctx.training), ctx.eps, int(ctx.relu), CF._ptr(dr), C, CF._ptr(ws), ws_n,
                                                 CF._stream()), "csn_rows_bn_act_bwd_f32")
        else:
            G = group_rows.numel() - 1
            ws_n = int(L.csn_rows_bn_act_groups_workspace_bytes(N, C, M, G))
            ws = _mc._workspace(ws_n, dev)
            _lib.check(L.csn_rows_bn_act_groups_bwd_f32(*head, group_rows.data_ptr(), G, int(ctx.relu), CF._ptr(dr), C, CF._ptr(ws), ws_n,
                                                        CF._stream()), "csn_rows_bn_act_groups_bwd_f32")
        return (None, None, None, None, dr, *outs)


Term = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]      # z, mean, scale, gamma, beta


# ------------------------------------------------------------------------------------------------------
# training on bf16 activation maps (section 28, ``tuning.train_maps16``)
# ------------------------------------------------------------------------------------------------------
_TRAIN16 = ('bf16 training maps need math mode "bf16" together with tuning.override(rows_single_product=True): only there does the '
            "fp32 form round these maps to bf16 itself")


class Map16:
    """A ReLU output of the training graph stored as bf16 rows (``bn_act(..., out_dtype=torch.bfloat16)``).

    ``rows`` (N, C) ``bfloat16``: the values, without autograd history.  ``edge`` (N, C) ``float32`` with ONE element of storage
    (``torch.zeros(1).expand(N, C)``): the map's place in the autograd graph.  Autograd casts a gradient to the dtype of the tensor
    it belongs to, so a bf16 tensor that required grad would receive its gradients rounded to bf16; the consumers (``conv_stats``,
    ``bn_act``'s residual) therefore read ``rows`` and return their fp32 ``dx`` / ``dr`` for ``edge``, whose several gradients autograd
    sums in fp32 as it does for an fp32 map.  No fp32 copy of the map exists."""

    __slots__ = ("rows", "edge")

    def __init__(self, rows: torch.Tensor, edge: torch.Tensor):
        if rows.dtype != torch.bfloat16:
            raise ValueError(f"training maps are bfloat16, not {rows.dtype}: math mode \"fp16\" runs its backward in bf16, which would "
                             "round an fp16 map a second time")
        if rows.dim() != 2 or edge.dtype != torch.float32 or tuple(edge.shape) != tuple(rows.shape):
            raise ValueError("rows must be (N, C) bfloat16 and edge an fp32 tensor of the same shape")
        self.rows, self.edge = rows, edge

    shape = property(lambda self: self.rows.shape)
    is_cuda = property(lambda self: self.rows.is_cuda)

    def detach(self) -> torch.Tensor:
        """The stored rows (what ``trace`` receives)."""
        return self.rows.detach()


def train_maps16_open() -> bool:
    """Whether section 28 takes calls right now: math mode "bf16" with ``tuning.rows_single_product``."""
    return tuning.current().rows_single_product and CF.current_mode() == 2


def _need_train16(*maps: Optional[Map16]) -> None:
    """The gate of the section-28 calls: the mode first, then the device."""
    if not train_maps16_open():
        raise ValueError(_TRAIN16)
    for m in maps:
        if m is not None and not m.is_cuda:
            raise _lib.CsnError(_NO_CPU)


class _ConvStats16(torch.autograd.Function):
    """``_ConvStats`` on a ``Map16`` (``csn_sparse_conv_stats_fwd_t16`` / ``csn_sparse_conv_bwd_t16``): the bf16 rows are gathered as
    they lie, forward and in the weight gradient; dx is fp32 and belongs to the map's edge."""

    @staticmethod
    def forward(ctx, x_rows, x_edge, w, kmap, running_mean, running_var, eps, momentum):
        CF._need_cuda(x_rows, w, kmap.fwd, running_mean, running_var, also=(torch.bfloat16,))
        L = _lib.lib()
        x = x_rows if _pitched16(x_rows) else x_rows.contiguous()
        w_c = w.detach().contiguous()
        KV, c_in, c_out = w_c.shape
        n_in, n_out = kmap.n_in, kmap.n_out
        ws_n = int(L.csn_sparse_conv_stats_workspace_bytes(n_out, c_out))
        z, mean, invstd, ws = _stats_outputs(n_out, c_out, ws_n, x.device)
        with CF.rows16(True):
            _lib.check(L.csn_sparse_conv_stats_fwd_t16(CF._ptr(x), 1, x.stride(0), n_in, CF._ptr(kmap.fwd), n_out, KV, c_in, c_out, CF._ptr(w_c),
                                                       CF._ptr(z), c_out, CF._ptr(mean), CF._ptr(invstd), CF._ptr(running_mean),
                                                       CF._ptr(running_var), float(eps), float(momentum), CF._ptr(ws), ws_n, CF._stream()),
                       "csn_sparse_conv_stats_fwd_t16")
        ctx.save_for_backward(x, w_c)
        ctx.kmap = kmap
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dmean, _dinvstd):
        need_x, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_x or need_w):
            return (None,) * 8
        with CF.math_mode(2), CF.rows16(True):
            x, w = ctx.saved_tensors
            dx, dw, _ = _mc._sparse_conv_backward(dz, x, x.stride(0), w, ctx.kmap, need_x, need_w)
        return (None, dx, dw) + (None,) * 5


def _conv_stats16(x: Map16, weight, kmap, running_mean, running_var, eps, momentum):
    _need_train16(x)
    if not weight.is_cuda:
        raise _lib.CsnError(_NO_CPU)
    if weight.dim() != 3 or x.shape[1] != weight.shape[1] or weight.shape[0] != kmap.KV or x.shape[0] != kmap.n_in:
        raise ValueError("x must be (n_in, c_in) and weight (KV, c_in, c_out) for the map's KV and n_in")
    c_in, c_out = weight.shape[1], weight.shape[2]
    if c_out % 32 or not 32 <= c_out <= 256 or c_in % 32 or not 32 <= c_in <= 256:
        raise ValueError("widths: c_out and a bf16 map's c_in multiples of 32 in [32, 256]")
    if kmap.n_out == 1:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    return _ConvStats16.apply(x.rows, x.edge, weight, kmap, running_mean, running_var, eps, momentum)


class _BnAct16(torch.autograd.Function):
    """``_BnAct`` with the residual read from and / or the result written as bf16 rows (``csn_rows_bn_act_fwd_t16`` / ``_bwd_t16``; the
    whole map is one batch).  ``r_rows`` / ``r_edge``: a ``Map16`` residual's two tensors, or (None, an fp32 residual), or (None,
    None).  ``out16``: returns (rows bf16, edge) — the parts of a ``Map16`` — instead of y fp32.  Arguments after the fixed ones:
    (z, mean, scale, gamma, beta) per term."""

    @staticmethod
    def forward(ctx, relu, training, eps, out16, r_rows, r_edge, *flat):
        M = len(flat) // 5
        CF._need_cuda(r_rows, *flat, also=(torch.bfloat16,))
        L = _lib.lib()
        zs, means, scales, gammas, betas = _bn_unpack(flat, training)
        N, C = zs[0].shape
        if r_rows is not None:
            r_c = r_rows if _pitched16(r_rows) else r_rows.contiguous()
        else:
            r_c = None if r_edge is None else _rows(r_edge)
        y = torch.empty((N, C), device=zs[0].device, dtype=torch.bfloat16 if out16 else torch.float32)
        t = _bn_terms(zs, means, scales, gammas, betas=betas)
        with CF.rows16(True):
            _lib.check(L.csn_rows_bn_act_fwd_t16(ctypes.addressof(t), M, N, C, int(training), float(eps), CF._ptr(r_c), int(r_rows is not None),
                                                 0 if r_c is None else r_c.stride(0), int(relu), CF._ptr(y), int(out16), C, CF._stream()),
                       "csn_rows_bn_act_fwd_t16")
        ctx.save_for_backward(y if relu else None, *zs, *means, *scales, *gammas)
        ctx.M, ctx.relu, ctx.training, ctx.eps, ctx.out16 = M, bool(relu), bool(training), float(eps), bool(out16)
        ctx.has_r = r_c is not None
        if not out16:
            return y
        ctx.mark_non_differentiable(y)
        return y, _zero_vec(y.device, 1).expand(N, C)                       # (one cached word: no launch, nothing is ever written)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        dy = grads[-1]                                                      # out16: (the rows' None, the edge's gradient)
        M = ctx.M
        saved = ctx.saved_tensors
        y = saved[0]
        zs, means, scales, gammas = (saved[1 + k * M:1 + (k + 1) * M] for k in range(4))
        L = _lib.lib()
        N, C = zs[0].shape
        dev = dy.device
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dr = torch.empty((N, C), device=dev, dtype=torch.float32) if (ctx.has_r and need[5]) else None
        grads, outs = _bn_grads(need, 6, M, N, C, dev)
        t = _bn_terms(zs, means, scales, gammas, grads=grads)
        ws_n = int(L.csn_rows_bn_act_workspace_bytes(N, C, M))
        ws = _mc._workspace(ws_n, dev)
        with CF.math_mode(2), CF.rows16(True):
            _lib.check(L.csn_rows_bn_act_bwd_t16(CF._ptr(dy), C, CF._ptr(y), int(ctx.out16), C, ctypes.addressof(t), M, N, C, int(ctx.training),
                                                 ctx.eps, int(ctx.relu), CF._ptr(dr), C, CF._ptr(ws), ws_n, CF._stream()),
                       "csn_rows_bn_act_bwd_t16")
        return (None, None, None, None, None, dr, *outs)


# ------------------------------------------------------------------------------------------------------
# inference: convolution + BatchNorm + residual + ReLU as one launch (section 19)
# ------------------------------------------------------------------------------------------------------
_WINDOW = 0x7fffffff                                  # bytes of a map (rows * pitch * 4) the kernels' gathers can address


def _pitched(t: torch.Tensor) -> bool:
    """Whether the kernels can take the fp32 rows ``t (n, c)`` where they lie: unit column stride, a row pitch that is a multiple
    of 4 floats and at least the width, a 16-byte aligned first element."""
    return (t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1]
            and t.data_ptr() % 16 == 0)


_DTYPES16 = (torch.bfloat16, torch.float16)
_MODE_DTYPE16 = {2: torch.bfloat16, 3: torch.float16}  # the 16-bit map type of a math mode (CSN_MATH_BF16 / CSN_MATH_FP16)


def _pitched16(t: torch.Tensor) -> bool:
    """``_pitched`` for bf16 / fp16 rows: a row pitch that is a multiple of 8 elements (16 bytes) and at least the width, a 16-byte
    aligned first element."""
    return (t.dtype in _DTYPES16 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= t.shape[1]
            and t.data_ptr() % 16 == 0)


def _rows(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().float()
    return t if _pitched(t) else t.contiguous()


def _rows_any(t: torch.Tensor) -> torch.Tensor:
    """``_rows`` that leaves 16-bit rows in their type."""
    if t.dtype not in _DTYPES16:
        return _rows(t)
    t = t.detach()
    return t if _pitched16(t) else t.contiguous()


def maps16_dtype() -> Optional[torch.dtype]:
    """The dtype 16-bit maps have right now — ``bfloat16`` in math mode "bf16", ``float16`` in "fp16", each with
    ``tuning.rows_single_product`` — or None where section 24 has no instance (every other mode, or the switch off)."""
    if not tuning.current().rows_single_product:
        return None
    return _MODE_DTYPE16.get(CF.current_mode())


def _maps16_route(x, residual, out, out_dtype) -> Optional[torch.dtype]:
    """None: an all-fp32 call (section 19).  Otherwise the 16-bit dtype of a section-24 call, checked against the math mode."""
    given = [t.dtype for t in (x, residual, out) if t is not None] + ([] if out_dtype is None else [out_dtype])
    if out_dtype is None and not any(d in _DTYPES16 for d in given):
        return None
    if out_dtype is not None and out_dtype not in (torch.float32,) + _DTYPES16:
        raise ValueError("out_dtype must be torch.float32, torch.bfloat16 or torch.float16")
    if out is not None and out_dtype is not None and out.dtype != out_dtype:
        raise ValueError("out_dtype differs from out's dtype")
    want = maps16_dtype()
    if want is None:
        raise ValueError('16-bit maps (a bfloat16 / float16 tensor, or out_dtype) need math mode "bf16" or "fp16" together with '
                         "tuning.override(rows_single_product=True)")
    other = [d for d in given if d in _DTYPES16 and d != want]
    if other:
        raise ValueError(f"the 16-bit maps of this math mode are {want}: got {other[0]}")
    return want


_ZEROS: Dict[Tuple[torch.device, int], torch.Tensor] = {}


def _zero_vec(device: torch.device, c: int) -> torch.Tensor:
    """``c`` fp32 zeros on ``device``, made once (never written)."""
    key = (device, c)
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(c, device=device, dtype=torch.float32)
    return _ZEROS[key]


def sparse_conv_bn_act(x: torch.Tensor, weight: torch.Tensor, kmap: KernelMap, norm: nn.BatchNorm1d,
                       residual: Optional[torch.Tensor] = None, relu: bool = True, out: Optional[torch.Tensor] = None, *,
                       shift: bool = True, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``y (n_out, c_out) = act(conv(x) s + t + residual)`` in one launch (``csn_sparse_conv_bn_act_fwd_f32``): ``conv`` the
    convolution ``kmap`` describes without a bias, ``s = gamma / sqrt(running_var + eps)``, ``t = beta - running_mean s`` from
    ``norm``'s running statistics, ``act`` the ReLU or the identity.  Inference only: no autograd node, the result has no ``grad_fn``.

    ``x``, ``residual`` and ``out`` may be row-pitched views of a wider buffer (``stride(1) == 1``, ``stride(0) % 4 == 0``, a
    16-byte aligned data pointer); ``x`` and ``residual`` are made contiguous otherwise, ``out`` raises ``ValueError``.  With
    ``out`` the result is written there (a column block of a wider buffer keeps its other columns) and ``out`` is returned;
    ``residual`` may be ``out`` itself — a sum that accumulates in place — and must not overlap it in any other way.  An input width
    that is no multiple of 32 is zero-padded as in ``sparse_conv3d``.  ``shift=False`` hands the launch zero ``beta`` and
    ``running_mean`` vectors (``t = 0``): the later launches of a chain that adds the products of an input's column blocks in place.

    16-bit maps (``csn_sparse_conv_bn_act_fwd_m16``, section 24).  In math mode "bf16" / "fp16" with ``tuning.rows_single_product``,
    ``x``, ``residual`` and ``out`` may each be fp32 or that mode's 16-bit dtype (``bfloat16`` / ``float16``; 16-bit views need
    ``stride(0) % 8 == 0``), and ``out_dtype`` names the type of a result allocated here.  Any 16-bit tensor, or an ``out_dtype``
    (``torch.float32`` included: all-fp32 maps on section 24's instances, the bits of section 19), takes that route; without the
    mode and the switch, or with a tensor of the other 16-bit type, it raises ``ValueError``.  The launch is bit-identical to the
    fp32 one on the same values, its result rounded once (nearest even) where the output is 16-bit.  Calls on fp32 tensors without
    ``out_dtype`` are section 19 as ever."""
    dt16 = _maps16_route(x, residual, out, out_dtype)
    if not (x.is_cuda and weight.is_cuda) or (residual is not None and not residual.is_cuda) or (out is not None and not out.is_cuda):
        raise _lib.CsnError(_NO_CPU)
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1] or weight.shape[0] != kmap.KV or x.shape[0] != kmap.n_in:
        raise ValueError("x must be (n_in, c_in) and weight (KV, c_in, c_out) for the map's KV and n_in")
    KV, c_in, c_out = weight.shape
    if c_out % 32 or not 32 <= c_out <= 256 or c_in > 256:
        raise ValueError("widths: c_out a multiple of 32 in [32, 256], c_in at most 256")
    if not isinstance(norm, nn.BatchNorm1d) or norm.num_features != c_out or norm.running_mean is None or norm.weight is None:
        raise ValueError(f"norm must be an affine nn.BatchNorm1d({c_out}) that tracks running statistics")
    n_in, n_out = kmap.n_in, kmap.n_out
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and tuple(t.shape) != (n_out, c_out):
            raise ValueError(f"{name} must be ({n_out}, {c_out})")
    CF._need_cuda(kmap.fwd, norm.weight, norm.bias, norm.running_mean, norm.running_var)
    same = residual is not None and out is not None and residual.data_ptr() == out.data_ptr() and residual.stride() == out.stride()
    w = weight.detach().float()
    x = x.detach() if x.dtype in _DTYPES16 else x.detach().float()
    pad = -c_in % 32
    if pad:
        x, w, c_in = F.pad(x, (0, pad)), F.pad(w, (0, 0, 0, pad)), c_in + pad
    x, w = _rows_any(x), w.contiguous()
    if out is None:
        y = torch.empty((n_out, c_out), device=x.device, dtype=out_dtype or torch.float32)
    else:
        y = out.detach()
        if not (_pitched(y) or (dt16 is not None and _pitched16(y))):
            raise ValueError("out must be fp32 rows with stride(1) == 1, stride(0) % 4 == 0 and a 16-byte aligned data pointer"
                             + ("" if dt16 is None else f", or {dt16} rows with stride(0) % 8 == 0"))
    r = None if residual is None else (y if same else _rows_any(residual))
    vec = [v.detach().float().contiguous() for v in (norm.weight, norm.bias, norm.running_mean, norm.running_var)]
    if not shift:
        vec[1] = vec[2] = _zero_vec(x.device, c_out)
    if dt16 is not None:
        is16 = lambda t: int(t is not None and t.dtype == dt16)
        with CF.rows16(True):
            _lib.check(_lib.lib().csn_sparse_conv_bn_act_fwd_m16(
                CF._ptr(x), is16(x), x.stride(0), n_in, CF._ptr(kmap.fwd), n_out, KV, c_in, c_out, CF._ptr(w), *(CF._ptr(v) for v in vec),
                float(norm.eps), CF._ptr(r), is16(r), 0 if r is None else r.stride(0), int(bool(relu)), CF._ptr(y), is16(y), y.stride(0),
                CF._stream()), "csn_sparse_conv_bn_act_fwd_m16")
        return y if out is None else out
    with CF.rows16(tuning.current().rows_single_product):
        _lib.check(_lib.lib().csn_sparse_conv_bn_act_fwd_f32(
            CF._ptr(x), x.stride(0), n_in, CF._ptr(kmap.fwd), n_out, KV, c_in, c_out, CF._ptr(w), *(CF._ptr(v) for v in vec),
            float(norm.eps), CF._ptr(r), 0 if r is None else r.stride(0), int(bool(relu)), CF._ptr(y), y.stride(0), CF._stream()),
            "csn_sparse_conv_bn_act_fwd_f32")
    return y if out is None else out


def _fits(layer: SparseConv3d, kmap: KernelMap) -> None:
    if kmap.kernel_size != layer.kernel_size or kmap.stride != layer.stride or kmap.transposed != layer.transposed:
        raise ValueError("the map does not fit this layer")


def _conv_bn_act(conv: SparseConv3d, norm: nn.BatchNorm1d, x, kmap: KernelMap, residual=None, relu=True, out=None,
                 out_dtype=None) -> torch.Tensor:
    _fits(conv, kmap)
    return sparse_conv_bn_act(x, conv.kernel, kmap, norm, residual, relu, out, out_dtype=out_dtype)


def _bn_act(terms: Sequence[Term], grouped: bool, group_rows, residual, relu, training, eps, out_dtype=None):
    if not 1 <= len(terms) <= 3:
        raise ValueError(("bn_act_groups" if grouped else "bn_act") + " takes 1 to 3 terms")
    m16 = isinstance(residual, Map16) or out_dtype is not None            # a section-28 call
    if m16:
        if grouped:
            raise ValueError("row groups have no bf16-map form (include/csn_hip.h section 28 takes the whole map as one batch)")
        if out_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, not {out_dtype}: math mode \"fp16\" runs its backward "
                             "in bf16, which would round an fp16 map a second time")
        _need_train16(residual if isinstance(residual, Map16) else None)
    flat = []
    N, C = terms[0][0].shape
    G = None
    if grouped:                                       # every map's device before the offsets' own checks
        for z, *_ in terms:
            if not z.is_cuda:
                raise _lib.CsnError(_NO_CPU)
        G = _check_groups(group_rows, terms[0][0])
    for z, mean, scale, gamma, beta in terms:
        if not grouped and not z.is_cuda:             # a term's device before its shapes
            raise _lib.CsnError(_NO_CPU)
        if tuple(z.shape) != (N, C) or any(v.numel() != C for v in (gamma, beta)) or any(
                v.numel() != C if G is None else tuple(v.shape) != (G, C) for v in (mean, scale)):
            raise ValueError("every term needs an (N, C) map and four (C,) vectors" if G is None else
                             "every term needs an (N, C) map, two (G, C) statistics and two (C,) vectors")
        flat += [z.float(), mean, scale, gamma, beta]
    if C % 32 or not 32 <= C <= 256:
        raise ValueError(f"width {C} is not supported: a multiple of 32 in [32, 256]")
    if residual is not None:
        if not residual.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if tuple(residual.shape) != (N, C):
            raise ValueError("the residual must be (N, C)")
        if not isinstance(residual, Map16):
            residual = residual.float()
    if m16:
        r_rows, r_edge = (residual.rows, residual.edge) if isinstance(residual, Map16) else (None, residual)
        out = _BnAct16.apply(bool(relu), bool(training), float(eps), out_dtype == torch.bfloat16, r_rows, r_edge, *flat)
        return Map16(*out) if out_dtype == torch.bfloat16 else out
    return _BnAct.apply(bool(relu), bool(training), float(eps), group_rows if grouped else None, residual, *flat)


def bn_act(terms: Sequence[Term], residual=None, relu: bool = True, training: bool = True, eps: float = 1e-5,
           out_dtype: Optional[torch.dtype] = None):
    """``y (N, C) = act(sum_m (gamma_m (z_m - mean_m) s_m + beta_m) + residual)`` for 1 to 3 terms ``(z, mean, scale, gamma, beta)``:
    training takes ``scale = invstd`` (of ``conv_stats``), eval the running mean / variance and ``eps``.

    bf16 training maps (section 28; math mode "bf16" with ``tuning.rows_single_product``, else ``ValueError``): ``residual`` may be a
    ``Map16``, and ``out_dtype=torch.bfloat16`` returns one — the same y rounded once to bf16 (nearest even), whose backward masks
    on the stored value; ``out_dtype=torch.float32`` names an fp32 result on the same route.  Without either the call is section 15
    as ever."""
    return _bn_act(terms, False, None, residual, relu, training, eps, out_dtype)


def bn_act_groups(terms: Sequence[Term], group_rows: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = True,
                  eps: float = 1e-5) -> torch.Tensor:
    """``bn_act`` in training mode on rows that are G BatchNorm batches: for row i of group g (``group_rows`` as in
    ``conv_stats_groups``) ``y_i = act(sum_m (gamma_m (z_m,i - mean_m[g]) scale_m[g] + beta_m) + residual_i)`` for 1 to 3 terms
    ``(z (N, C), mean (G, C), scale (G, C) = invstd of conv_stats_groups, gamma (C,), beta (C,))``.  ``eps`` is part of the
    statistics already (kept for the signature of ``bn_act``).  The backward is the complete BatchNorm gradient per group."""
    return _bn_act(terms, True, group_rows, residual, relu, True, eps)


# ------------------------------------------------------------------------------------------------------
# conv + norm as a term; combining terms
# ------------------------------------------------------------------------------------------------------
def _conv_bn(conv: SparseConv3d, norm: nn.BatchNorm1d, x: torch.Tensor, kmap: KernelMap, fused: bool, groups=None):
    """fused: the term (z, mean, scale, gamma, beta) of ``bn_act``; else the normalised map through ATen.  ``groups`` (training,
    fused): the (group_rows, G) of the map's output level — the term of ``bn_act_groups``, the norm sees G batches."""
    _fits(conv, kmap)
    if groups is not None:
        if not x.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        norm.num_batches_tracked += groups[1]
        z, mean, invstd = conv_stats_groups(x, conv.kernel, kmap, groups[0], norm.running_mean, norm.running_var, norm.eps, norm.momentum)
        return (z, mean, invstd, norm.weight, norm.bias)
    training = norm.training
    if not x.is_cuda:
        raise _lib.CsnError(_NO_CPU)
    if training and kmap.n_out == 1:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    if not fused:
        return norm(sparse_conv3d(x, conv.kernel, None, kmap))
    if training:
        norm.num_batches_tracked += 1
        z, mean, invstd = conv_stats(x, conv.kernel, kmap, norm.running_mean, norm.running_var, norm.eps, norm.momentum)
        return (z, mean, invstd, norm.weight, norm.bias)
    return (sparse_conv3d(x, conv.kernel, None, kmap), norm.running_mean, norm.running_var, norm.weight, norm.bias)


def _combine(parts: Sequence, fused: bool, training: bool, eps: float = 1e-5, groups=None, out_dtype=None):
    """relu(sum of ``parts``) where a part is a term / normalised map of ``_conv_bn`` or ("r", map) for a plain map.  The ATen path
    adds in the order given (the reference's, hrnet.py:157-161).  ``groups``: as in ``_conv_bn``, for the level of the sum.
    ``out_dtype`` (fused, ``tuning.train_maps16``): ``bn_act``'s."""
    if fused:
        terms = [p for p in parts if not (isinstance(p, tuple) and p[0] == "r")]
        res = [p[1] for p in parts if isinstance(p, tuple) and p[0] == "r"]
        if not terms:
            # the finest branch after stage 0 has no incoming path: the reference's ReLU of a block's output, itself a ReLU
            # output — the same values, and the same gradient (the block's own mask zeroes the same elements): no launch
            return res[0]
        if groups is not None:
            return bn_act_groups(terms, groups[0], res[0] if res else None, True, eps)
        return bn_act(terms, res[0] if res else None, True, training, eps, out_dtype)
    maps = [p[1] if isinstance(p, tuple) else p for p in parts]
    buf = maps[0]
    for m in maps[1:]:
        buf = buf + m
    return F.relu(buf)


def _keep(trace: Optional[Dict[str, torch.Tensor]], name: str, y: torch.Tensor) -> torch.Tensor:
    if trace is not None:
        trace[name] = y.detach()
    return y


class HRBasicBlock(nn.Module):
    """``BasicBlock`` of resnet_block.py:22-57 without a downsample (the backbone has none), on the fused nodes.  State-dict keys
    are those of ``SparseBasicBlock``: ``conv1.kernel``, ``norm1.*``, ``conv2.kernel``, ``norm2.*``.  ``trace`` (a dict) receives the
    two ReLU outputs under ``prefix + "norm1"`` / ``prefix + "norm2"``."""

    expansion = 1

    def __init__(self, inplanes: int, planes: int, bn_momentum: float = 0.02, fused: bool = True):
        super().__init__()
        if inplanes != planes:
            raise ValueError("the backbone's blocks keep their width (no downsample)")
        self.conv1 = SparseConv3d(inplanes, planes, kernel_size=3, stride=1)
        self.norm1 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.conv2 = SparseConv3d(planes, planes, kernel_size=3, stride=1)
        self.norm2 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.fused = fused

    def forward(self, x, kmap: KernelMap, trace: Optional[dict] = None, prefix: str = "", group_rows: Optional[torch.Tensor] = None,
                dtype: Optional[torch.dtype] = None, out_dtype: Optional[torch.dtype] = None):
        """``group_rows`` (training, fused): the rows are G BatchNorm batches (``conv_stats_groups``).  ``dtype`` / ``out_dtype``
        (training, fused, ``tuning.train_maps16``): ``bn_act``'s ``out_dtype`` for the inner map and for the block's result —
        ``torch.bfloat16`` stores a ``Map16``; ``x`` may be one."""
        f, tr = self.fused, self.training
        g = None
        if group_rows is not None and tr:
            if not f:
                raise ValueError("row groups in training need fused=True: ATen has no grouped BatchNorm")
            g = (group_rows, group_rows.numel() - 1)
        out = _keep(trace, prefix + "norm1", _combine([_conv_bn(self.conv1, self.norm1, x, kmap, f, g)], f, tr, self.norm1.eps, g, dtype))
        t2 = _conv_bn(self.conv2, self.norm2, out, kmap, f, g)
        return _keep(trace, prefix + "norm2", _combine([t2, ("r", x)], f, tr, self.norm2.eps, g, out_dtype))

    def infer(self, x: torch.Tensor, kmap: KernelMap, trace: Optional[dict] = None, prefix: str = "",
              out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None,
              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """The block on the inference launches: two, the second with ``x`` as its residual (written to ``out`` when given).
        ``dtype`` (16-bit inference maps, ``tuning.infer_maps16``): the type of the inner map; ``out_dtype``: that of the block's
        result (``out``'s own when given)."""
        h = _keep(trace, prefix + "norm1", _conv_bn_act(self.conv1, self.norm1, x, kmap, out_dtype=dtype))
        return _keep(trace, prefix + "norm2", _conv_bn_act(self.conv2, self.norm2, h, kmap, residual=x, out=out, out_dtype=out_dtype))


# ------------------------------------------------------------------------------------------------------
# the backbone
# ------------------------------------------------------------------------------------------------------
class HRNetBackbone(nn.Module):
    """``HRNetBase.backbone_initialization`` + ``forward_backbone`` + the final transitions + the concatenation (hrnet.py:31-163,
    308-326, 433-437) with the reference's module names: ``conv0s1``, ``bn0s1``, ``conv1s1``, ``bn1s1``, ``stages.i.j.b``,
    ``exchange_blocks.i.j.k.*`` (sequential indices with the ReLUs counted: a two-step path has conv 0, norm 1, relu 2, conv 3, norm
    4), ``final_transitions.i.*`` (conv 3s, norm 3s + 1, relu 3s + 2).

    ``forward(feats, pyramid, trace=None)``: ``feats (N, in_channels)`` on the pyramid's level-0 rows; returns the
    ``(N, init_dim + sum of the branch widths)`` rows [out_init | branch 0 | transition 1 | ...].  ``trace``: a dict that receives
    every ReLU's output, keyed ``bn0s1``, ``bn1s1``, ``stages.i.j.b.norm1`` / ``.norm2``, ``exchange_blocks.i.j.k.<norm index>``
    (the inner steps of a multi-step path), ``sum.i.k`` (the branch sums after stage i) and ``final_transitions.i.<norm index>``.

    ``pyramid`` may be a ``GroupedPyramid`` (G batches merged, ``merge_batches``): in training every BatchNorm then takes its
    statistics per group (``conv_stats_groups`` / ``bn_act_groups``; ``num_batches_tracked`` advances by G, the running statistics
    see the groups in order; ``fused=False`` raises ``ValueError``), in eval mode the pass is the one below on the merged pyramid.

    Under ``tuning.override(eval_epilogue=True)`` a fused backbone in eval mode, called with autograd disabled, runs the inference
    graph (``_forward_infer``); in every other case the switch changes nothing.

    Under ``tuning.override(train_maps16=True)`` a fused backbone in training mode, on a plain ``VoxelPyramid`` in math mode "bf16"
    with ``rows_single_product``, stores as bf16 rows (``Map16``) every ReLU output that only its own nodes read: ``bn1s1``, the inner
    and outer outputs of the blocks, the branch sums, the inner steps of the exchange paths and of the final transitions.  ``bn0s1``,
    branch 0's last block output and the last step of each final transition — what ``torch.cat`` joins — stay fp32, as do z, the
    statistics and every gradient; ``trace`` receives the maps as stored.  The step equals the fp32-map step with every stored map
    rounded once.  Math modes "fp16" (its backward runs in bf16 and would round an fp16 map again), "fp32" and "bf16x3",
    ``rows_single_product`` off, ``fused=False``, a ``GroupedPyramid`` and eval mode — of the backbone or of any of its submodules (a
    frozen block or BatchNorm) — ignore the switch: the same calls, the same bits."""

    NUM_BLOCKS = 3

    def __init__(self, in_channels: int = 3, num_stages: int = 3, feat_factor: int = 2, init_dim: int = 32, conv1_kernel_size: int = 5,
                 bn_momentum: float = 0.02, fused: bool = True):
        super().__init__()
        D = init_dim * feat_factor
        if D * 2 ** (num_stages - 1) > 256:
            raise NotImplementedError(f"the coarsest branch would be {D * 2 ** (num_stages - 1)} wide: the convolution kernels "
                                      "(include/csn_hip.h section 14) take widths up to 256")
        self.num_stages, self.init_dim, self.init_stage_dims, self.fused = num_stages, init_dim, D, fused
        self.conv1_kernel_size = conv1_kernel_size
        bn = lambda c: nn.BatchNorm1d(c, momentum=bn_momentum)
        self.conv0s1 = SparseConv3d(in_channels, init_dim, kernel_size=conv1_kernel_size)
        self.bn0s1 = bn(init_dim)
        self.conv1s1 = SparseConv3d(init_dim, D, kernel_size=3)
        self.bn1s1 = bn(D)
        self.stages, self.exchange_blocks = nn.ModuleList(), nn.ModuleList()
        for i in range(num_stages):
            self.stages.append(nn.ModuleList(
                nn.ModuleList(HRBasicBlock(D * 2 ** j, D * 2 ** j, bn_momentum, fused) for _ in range(self.NUM_BLOCKS))
                for j in range(i + 1)))
            if i == num_stages - 1:
                break
            depth = i + 1
            ex = nn.ModuleList()
            for j in range(depth):
                row = nn.ModuleList()
                c0 = D * 2 ** j
                for k in range(depth + 1):
                    path = nn.ModuleList()
                    for s in range(abs(k - j)):
                        if s:
                            path.append(nn.ReLU())
                        if k > j:
                            path.append(SparseConv3d(c0 * 2 ** s, c0 * 2 ** (s + 1), kernel_size=3, stride=2))
                            path.append(bn(c0 * 2 ** (s + 1)))
                        else:
                            path.append(SparseConvTranspose3d(c0 // 2 ** s, c0 // 2 ** (s + 1)))
                            path.append(bn(c0 // 2 ** (s + 1)))
                    row.append(path)
                ex.append(row)
            self.exchange_blocks.append(ex)
        self.final_transitions = nn.ModuleList()
        for i in range(1, num_stages):
            c = D * 2 ** i
            block = nn.ModuleList()
            for _ in range(i):
                block += [SparseConvTranspose3d(c, c), bn(c), nn.ReLU()]
            self.final_transitions.append(block)
        self.out_channels = init_dim + sum(D * 2 ** s for s in range(num_stages))
        for m in self.modules():                                            # hrnet.py:165-169
            if isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def forward(self, feats: torch.Tensor, pyramid, trace: Optional[dict] = None) -> torch.Tensor:
        if not feats.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        grp = None                                                          # level -> (group_rows, G): training on a GroupedPyramid
        if isinstance(pyramid, GroupedPyramid):
            # eval: the running statistics do not depend on the group — the existing path on the merged pyramid
            if self.training:
                if not self.fused:
                    raise ValueError("a GroupedPyramid in training needs fused=True: ATen has no grouped BatchNorm")
                grp = pyramid.groups
            pyramid = pyramid.pyramid
        if pyramid.n_levels < self.num_stages or pyramid.stem_kernel != self.conv1_kernel_size:
            raise ValueError(f"the pyramid needs {self.num_stages} levels and a kernel-{self.conv1_kernel_size} stem map")
        if feats.dim() != 2 or feats.shape[0] != pyramid.coords[0].shape[0]:
            raise ValueError("feats must be (N, in_channels) rows of the pyramid's level 0")
        f, tr = self.fused, self.training
        if tuning.current().eval_epilogue and f and not tr and not torch.is_grad_enabled():
            return self._forward_infer(feats, pyramid, trace)
        G = (lambda level: None) if grp is None else grp                    # the groups of a map on `level`
        # tuning.train_maps16: the stored maps' out_dtype (bf16 rows, Map16) and that of the maps torch.cat joins (fp32 on the
        # same route); None: every map fp32 on section 15, the calls as ever.  A backbone with a submodule in eval mode (a frozen
        # block or BatchNorm: that layer runs sparse_conv3d on the running statistics) is not in training mode for this purpose
        on16 = (tuning.current().train_maps16 and f and tr and grp is None and train_maps16_open()
                and all(m.training for m in self.modules()))
        m16, f32 = (torch.bfloat16, torch.float32) if on16 else (None, None)
        act1 = lambda name, t, level, dt=None: _keep(trace, name, _combine([t], f, tr, groups=G(level), out_dtype=dt))
        out_init = act1("bn0s1", _conv_bn(self.conv0s1, self.bn0s1, feats.float(), pyramid.stem, f, G(0)), 0)
        out = act1("bn1s1", _conv_bn(self.conv1s1, self.bn1s1, out_init, pyramid.s1[0], f, G(0)), 0, m16)
        stage_input = [out]
        for i in range(self.num_stages):
            stage_output = []
            for j in range(i + 1):
                x = stage_input[j]
                for b, blk in enumerate(self.stages[i][j]):
                    last = i == self.num_stages - 1 and j == 0 and b == len(self.stages[i][j]) - 1     # torch.cat reads it
                    x = blk(x, pyramid.s1[j], trace, f"stages.{i}.{j}.{b}.", None if grp is None else grp(j)[0], m16,
                            f32 if last else m16)
                stage_output.append(x)
            if i == self.num_stages - 1:
                break
            depth = i + 1
            stage_input = []
            for k in range(depth + 1):
                parts = []
                for j in range(depth):
                    if j == k:
                        parts.append(("r", stage_output[j]))
                        continue
                    path, x, steps = self.exchange_blocks[i][j][k], stage_output[j], abs(k - j)
                    for s in range(steps):
                        level = j + s if k > j else j - s                  # the level the step starts from
                        kmap = pyramid.down[level] if k > j else pyramid.up(level - 1)
                        to = level + 1 if k > j else level - 1             # the level the step ends on
                        t = _conv_bn(path[3 * s], path[3 * s + 1], x, kmap, f, G(to))
                        if s + 1 < steps:
                            x = act1(f"exchange_blocks.{i}.{j}.{k}.{3 * s + 1}", t, to, m16)
                        else:
                            parts.append(t)
                stage_input.append(_keep(trace, f"sum.{i}.{k}", _combine(parts, f, tr, groups=G(k), out_dtype=m16)))
        outs = [out_init, stage_output[0]]
        for i in range(1, self.num_stages):
            x, block = stage_output[i], self.final_transitions[i - 1]
            for s in range(i):
                x = act1(f"final_transitions.{i - 1}.{3 * s + 1}",
                         _conv_bn(block[3 * s], block[3 * s + 1], x, pyramid.up(i - s - 1), f, G(i - s - 1)), i - s - 1,
                         f32 if s == i - 1 else m16)
            outs.append(x)
        return torch.cat(outs, dim=1)

    def _forward_infer(self, feats: torch.Tensor, pyramid: VoxelPyramid, trace: Optional[dict]) -> torch.Tensor:
        """The same network with one launch per convolution + norm (``sparse_conv_bn_act``).  Every ReLU output is a stored map.
        A branch sum is a chain into one buffer, over the incoming paths in ascending source branch j: the first launch writes
        ``z s + t + own`` (``own``: the branch's own map, when it has one) without a ReLU, every further one adds its ``z s + t``
        to that buffer in place, the last applies the ReLU — ((own + p_0) + p_1) + ..., a summation order of its own.  The
        (N, out_channels) result is allocated once; ``bn0s1``, branch 0's last block and the last step of every final transition
        write their column blocks of it, and ``conv1s1`` reads ``out_init`` from there through the row pitch.  Where that pitch
        would take the result past the kernels' 2 GiB window, the maps stay separate and are joined with ``torch.cat``.

        Under ``tuning.infer_maps16`` in math mode "bf16" / "fp16" with ``rows_single_product`` (``maps16_dtype``), every map that
        is not a column block of the result is allocated, written and gathered in the mode's 16-bit dtype (section 24; every launch
        is ``csn_sparse_conv_bn_act_fwd_m16``): the same products, each stored map rounded once after the launch that writes it, a
        branch sum rounded per launch in its 16-bit buffer.  The stem's input, the result and the launches that write its column
        blocks stay fp32 (so does ``torch.cat``'s input past the window); ``trace`` receives the maps as stored."""
        m16 = maps16_dtype() if tuning.current().infer_maps16 else None     # the stored maps' dtype, or None: fp32 on section 19
        f32 = None if m16 is None else torch.float32                        # a result column's out_dtype under the switch
        n, D, S = feats.shape[0], self.init_stage_dims, self.num_stages
        widths = [self.init_dim] + [D * 2 ** s for s in range(S)]
        wide = torch.empty((n, self.out_channels), device=feats.device, dtype=torch.float32) \
            if n * self.out_channels * 4 <= _WINDOW else None
        col = lambda m: None if wide is None else wide[:, sum(widths[:m]):sum(widths[:m + 1])]
        out_init = _keep(trace, "bn0s1", _conv_bn_act(self.conv0s1, self.bn0s1, feats, pyramid.stem, out=col(0), out_dtype=f32))
        stage_input = [_keep(trace, "bn1s1", _conv_bn_act(self.conv1s1, self.bn1s1, out_init, pyramid.s1[0], out_dtype=m16))]
        for i in range(S):
            stage_output = []
            for j in range(i + 1):
                x, blocks = stage_input[j], self.stages[i][j]
                for b, blk in enumerate(blocks):
                    last = i == S - 1 and j == 0 and b == len(blocks) - 1
                    x = blk.infer(x, pyramid.s1[j], trace, f"stages.{i}.{j}.{b}.", out=col(1) if last else None, dtype=m16,
                                  out_dtype=f32 if last else m16)
                stage_output.append(x)
            if i == S - 1:
                break
            depth = i + 1
            stage_input = []
            for k in range(depth + 1):
                buf = stage_output[k] if k < depth else None                # the branch's own map: the first launch's residual
                sources = [j for j in range(depth) if j != k]
                for j in sources:
                    path, x, steps = self.exchange_blocks[i][j][k], stage_output[j], abs(k - j)
                    for s in range(steps):
                        level = j + s if k > j else j - s                  # the level the step starts from
                        kmap = pyramid.down[level] if k > j else pyramid.up(level - 1)
                        if s + 1 < steps:
                            x = _keep(trace, f"exchange_blocks.{i}.{j}.{k}.{3 * s + 1}",
                                      _conv_bn_act(path[3 * s], path[3 * s + 1], x, kmap, out_dtype=m16))
                        else:
                            buf = _conv_bn_act(path[3 * s], path[3 * s + 1], x, kmap, residual=buf, relu=j == sources[-1],
                                               out=None if j == sources[0] else buf, out_dtype=m16)
                # (no incoming path — the finest branch after stage 0 — is the block's own ReLU output: no launch, as in _combine)
                stage_input.append(_keep(trace, f"sum.{i}.{k}", buf))
        outs = [out_init, stage_output[0]]
        for i in range(1, S):
            x, block = stage_output[i], self.final_transitions[i - 1]
            for s in range(i):
                x = _keep(trace, f"final_transitions.{i - 1}.{3 * s + 1}",
                          _conv_bn_act(block[3 * s], block[3 * s + 1], x, pyramid.up(i - s - 1), out=col(i + 1) if s == i - 1 else None,
                                       out_dtype=f32 if s == i - 1 else m16))
            outs.append(x)
        return torch.cat(outs, dim=1) if wide is None else wide


# ------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------
Batch = Tuple[torch.Tensor, torch.Tensor]         # (coords (n, 4) sorted by shape — or a VoxelPyramid —, feats (n, in_channels))


class HRNetSimCSN(nn.Module):
    """``HRNetSimCSN`` (hrnet.py:296-454): ``backbone`` (``HRNetBackbone``) and ``head`` (``SimCSNHead`` with its ``fc_layer``).

    ``forward((coords, feats), keys=None, return_ssa=False)``: ``coords (N, 4)`` rows [b, x, y, z] sorted by shape (or a
    ``VoxelPyramid`` built for them), ``feats (N, in_channels)``; ``keys`` a list of K such batches, batch i holding the i-th
    neighbour of every query shape.  The backbone runs on the queries first and then on key batches 0 .. K-1, each its own
    BatchNorm batch, and so does ``fc_layer`` inside the head: per layer the running statistics see the batches in the reference's
    order (hrnet.py:425-454).  Returns the (N, out_channels) logits, or the SSA rows with ``return_ssa``."""

    NUM_STAGES = 1
    FEAT_FACTOR = 1

    def __init__(self, in_channels: int, out_channels: int, d_model: int = 256, n_head: int = 4, k_neighbors: int = 1,
                 dropout: float = 0.1, bn_momentum: float = 0.02, conv1_kernel_size: int = 5, init_dim: int = 32, fused: bool = True):
        super().__init__()
        self.backbone = HRNetBackbone(in_channels, self.NUM_STAGES, self.FEAT_FACTOR, init_dim, conv1_kernel_size, bn_momentum, fused)
        self.head = SimCSNHead(d_model, n_head, out_channels, k_neighbors, dropout=dropout,
                               backbone_channels=self.backbone.out_channels, bn_momentum=bn_momentum)

    def backbone_rows(self, batch: Batch):
        """(rows (N, backbone channels), offsets (B + 1)) of one batch."""
        where, feats = batch
        pyr = where if isinstance(where, VoxelPyramid) else build_pyramid(where, self.NUM_STAGES, self.backbone.conv1_kernel_size)
        if not feats.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if pyr.coords[0].device != feats.device:
            pyr = pyr.to(feats.device)
        return self.backbone(feats, pyr), offsets_from_batch_index(pyr.coords[0][:, 0])

    def _merged(self, queries: Batch, keys: Optional[Sequence[Batch]]) -> Optional[Tuple[GroupedPyramid, torch.Tensor]]:
        """The (GroupedPyramid, features) of a call that takes the grouped pass, or None for the separate passes: a
        ``GroupedPyramid`` given as the queries' coordinates; or ``tuning.grouped_passes`` with key batches, none of them a
        prebuilt ``VoxelPyramid`` (that cannot be merged after the fact), a backbone that can normalise groups (fused, or eval)
        and merged maps inside the kernels' 2 GiB gather window."""
        where, feats = queries
        if isinstance(where, GroupedPyramid):
            if keys:
                raise ValueError("a GroupedPyramid holds the key batches already: pass keys=None")
            return where, feats
        batches = [queries] + list(keys or [])
        if not (tuning.current().grouped_passes and keys) or len(batches) > MAX_GROUPS:
            return None
        if any(not isinstance(c, torch.Tensor) for c, _ in batches) or (self.training and not self.backbone.fused):
            return None
        if not all(f.is_cuda for _, f in batches):
            raise _lib.CsnError(_NO_CPU)
        # merged where the queries' coordinates live (host coordinates: the shape counts are free, the pyramid moves afterwards)
        dev = where.device
        gp = merge_batches([(c.to(dev), f) for c, f in batches], self.NUM_STAGES, self.backbone.conv1_kernel_size)
        D = self.backbone.init_stage_dims
        if any(gp.coords[l].shape[0] * D * 2 ** l * 4 > _WINDOW for l in range(self.NUM_STAGES)):
            return None
        return gp, torch.cat([f for _, f in batches])

    def forward(self, queries: Batch, keys: Optional[Sequence[Batch]] = None, return_ssa: bool = False):
        """With ``tuning.grouped_passes`` (or a ``GroupedPyramid`` and the concatenated features as ``queries``, ``keys=None``) the
        K + 1 batches run through the backbone as ONE pass over row groups — group 0 the queries, group 1 + i key batch i —
        and the head receives the groups' rows (one ``torch.split``) and offsets; ``fc_layer`` still runs once per group, in order."""
        merged = self._merged(queries, keys)
        if merged is None:
            q, qo = self.backbone_rows(queries)
            ks = [self.backbone_rows(b) for b in (keys or [])]
            return self.head(q, qo, keys=ks or None, return_ssa=return_ssa)
        gp, feats = merged
        if not feats.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if gp.coords[0].device != feats.device:
            gp = gp.to(feats.device)
        rows = self.backbone(feats, gp)
        host = gp.group_rows_host[0]
        parts = torch.split(rows, [b - a for a, b in zip(host, host[1:])])
        ks = [(parts[g], gp.group_offsets(g)) for g in range(1, gp.n_groups)]
        return self.head(parts[0], gp.group_offsets(0), keys=ks or None, return_ssa=return_ssa)


class HRNetSimCSN2S(HRNetSimCSN):
    NUM_STAGES, FEAT_FACTOR = 2, 4            # 32 + 128 + 256 = 416 backbone channels


class HRNetSimCSN3S(HRNetSimCSN):
    NUM_STAGES, FEAT_FACTOR = 3, 2            # 32 + 64 + 128 + 256 = 480 backbone channels


class HRNetSimCSN4S(HRNetSimCSN):
    NUM_STAGES, FEAT_FACTOR = 4, 2

    def __init__(self, *a, **kw):
        raise NotImplementedError("HRNetSimCSN4S needs 512-wide convolutions; the kernels (include/csn_hip.h section 14) take "
                                  "widths up to 256")


class SegFinal(BackboneFC):
    """``final`` of ``HRNetSeg`` (hrnet.py:246-262) with the reference's sequential indices: 0 / 1 / 2 the kernel-size-1
    convolution, BatchNorm and ReLU of ``BackboneFC`` (one autograd node on the fc_layer kernels), 3 the kernel-size-1 output
    convolution as an ``nn.Linear``."""

    WIDTH = 256

    def __init__(self, backbone_channels: int, out_channels: int, bn_momentum: float = 0.02):
        super().__init__(backbone_channels, self.WIDTH, bn_momentum=bn_momentum)
        self.append(nn.Linear(self.WIDTH, out_channels, bias=True))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.linear(super().forward(x), self[3].weight, self[3].bias)


class HRNetSeg(nn.Module):
    """``HRNetSeg`` (hrnet.py:214-275), the plain segmentation network: ``backbone`` (``HRNetBackbone``) and ``final``
    (``SegFinal``: ``final.0`` / ``.1`` / ``.2`` the 256-wide fc layer, ``final.3`` the output layer).

    ``forward((coords, feats))``: ``coords (N, 4)`` rows [b, x, y, z] (or a ``VoxelPyramid`` built for them), ``feats (N,
    in_channels)``; returns the (N, out_channels) logits, in training and eval."""

    NUM_STAGES = 1
    FEAT_FACTOR = 2

    def __init__(self, in_channels: int, out_channels: int, bn_momentum: float = 0.02, conv1_kernel_size: int = 5, init_dim: int = 32,
                 fused: bool = True):
        super().__init__()
        self.backbone = HRNetBackbone(in_channels, self.NUM_STAGES, self.FEAT_FACTOR, init_dim, conv1_kernel_size, bn_momentum, fused)
        self.final = SegFinal(self.backbone.out_channels, out_channels, bn_momentum)

    def forward(self, batch: Batch) -> torch.Tensor:
        where, feats = batch
        pyr = where if isinstance(where, VoxelPyramid) else build_pyramid(where, self.NUM_STAGES, self.backbone.conv1_kernel_size)
        if not feats.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if pyr.coords[0].device != feats.device:
            pyr = pyr.to(feats.device)
        return self.final(self.backbone(feats, pyr))


class HRNetSeg2S(HRNetSeg):
    NUM_STAGES = 2                            # 32 + 64 + 128 = 224 backbone channels


class HRNetSeg3S(HRNetSeg):
    NUM_STAGES = 3                            # 32 + 64 + 128 + 256 = 480 backbone channels


class HRNetSeg4S(HRNetSeg):
    NUM_STAGES = 4

    def __init__(self, *a, **kw):
        raise NotImplementedError("HRNetSimCSN4S needs 512-wide convolutions; the kernels (include/csn_hip.h section 14) take "
                                  "widths up to 256")


def _load_me_backbone(backbone: HRNetBackbone, state_dict) -> None:
    new = {}
    for name, mod in backbone.named_modules():
        if isinstance(mod, SparseConv3d):
            pairs = [(f"{name}.kernel", f"{name}.kernel", mod.kernel)]
        elif isinstance(mod, nn.BatchNorm1d):
            pairs = [(f"{name}.{p}", f"{name}.bn.{p}", getattr(mod, p))
                     for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        else:
            continue
        for own, ref, cur in pairs:
            if ref not in state_dict:
                raise ValueError(f"checkpoint has no {ref}")
            v = state_dict[ref]
            if tuple(v.shape) != tuple(cur.shape):
                raise ValueError(f"{ref} is {tuple(v.shape)}; expected {tuple(cur.shape)}")
            new[own] = v
    backbone.load_state_dict(new, strict=True)


def load_me_seg_state(model: HRNetSeg, state_dict) -> HRNetSeg:
    """Copy an ``HRNetSeg`` checkpoint of the reference into ``model``: the backbone as ``load_me_hrnet_state`` does; ``final`` as
    ``load_me_head_state`` maps ``fc_layer`` / ``output``: ``final.0.kernel`` and ``final.3.kernel`` — (c_in, c_out) or (1, c_in,
    c_out) — transposed into the ``nn.Linear`` weights, ``final.0.bias`` / ``final.3.bias`` — (c_out,) or (1, c_out) — flattened,
    ``final.1.bn.*`` into ``final.1.*``.  A missing key or a wrong shape raises ``ValueError`` before ``final`` is touched.  Parity
    of the KV-axis order is unpinned against MinkowskiEngine, as for every checkpoint here."""
    new = {}
    for i in (0, 3):
        c_out, c_in = model.final[i].weight.shape
        for need in (f"final.{i}.kernel", f"final.{i}.bias"):
            if need not in state_dict:
                raise ValueError(f"checkpoint has no {need}")
        kernel, bias = state_dict[f"final.{i}.kernel"], state_dict[f"final.{i}.bias"]
        if tuple(kernel.shape) == (1, c_in, c_out):
            kernel = kernel[0]
        if tuple(kernel.shape) != (c_in, c_out):
            raise ValueError(f"final.{i}.kernel is {tuple(kernel.shape)}; expected ({c_in}, {c_out}) or (1, {c_in}, {c_out})")
        if tuple(bias.shape) == (1, c_out):
            bias = bias[0]
        if tuple(bias.shape) != (c_out,):
            raise ValueError(f"final.{i}.bias is {tuple(bias.shape)}; expected ({c_out},) or (1, {c_out})")
        new[f"{i}.weight"], new[f"{i}.bias"] = kernel.t(), bias
    for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        ref = f"final.1.bn.{leaf}"
        if ref not in state_dict:
            raise ValueError(f"checkpoint has no {ref}")
        cur = getattr(model.final[1], leaf)
        if tuple(state_dict[ref].shape) != tuple(cur.shape):
            raise ValueError(f"{ref} is {tuple(state_dict[ref].shape)}; expected {tuple(cur.shape)}")
        new[f"1.{leaf}"] = state_dict[ref]
    _load_me_backbone(model.backbone, state_dict)
    model.final.load_state_dict(new, strict=True)
    return model


def load_me_hrnet_state(model: HRNetSimCSN, state_dict) -> HRNetSimCSN:
    """Copy an ``HRNetSimCSN`` checkpoint of the reference into ``model``.  The backbone's modules keep the reference's names
    (under ``backbone.`` here, at the top level there); a ``MinkowskiBatchNorm`` wraps its norm, so ``<name>.bn.weight`` etc. map
    to ``<name>.weight``; a convolution's ``<name>.kernel`` is (KV, c_in, c_out) on both sides.  The sequential indices of the
    exchange and transition blocks count the ReLUs on both sides.  The head goes through ``load_me_head_state``.  A missing key or
    a wrong shape raises ``ValueError``.  The order of the KV axis (the offset numbering of minkowski_conv.py) is this project's
    choice: parity unpinned against MinkowskiEngine."""
    from .minkowski_training import load_me_head_state
    _load_me_backbone(model.backbone, state_dict)
    load_me_head_state(model.head, state_dict)
    return model
