"""Sparse 3D convolution on voxel rows: the one primitive of MinkowskiNet's HRNet backbone, on the MI355X kernels.

Reference (marios2019/CSN):
  * the stem, the stride-2 / transposed convolutions between branches, the blocks   MinkowskiNet/models/hrnet.py:39-53, 89-111, 233-239
  * ``BasicBlock``                                                                 MinkowskiNet/models/modules/resnet_block.py:22-57

Features are point-major fp32 rows ``x (n, c)``; coordinates are integer rows ``coords (n, 4) = [b, x, y, z]``, unique, every
x, y, z a multiple of the tensor stride ``ts``.  For an odd kernel size k (r = k // 2, KV = k^3) the offsets o = (ox, oy, oz) in
[-r, r]^3 are numbered ``kidx = (ox + r) + k (oy + r) + k^2 (oz + r)`` (x fastest); the weight is ``(KV, c_in, c_out)``.

  * stride 1:             out coords = in coords,                        y[c]  = sum_o x[c  + ts o] W[kidx(o)]
  * stride 2, k = 3:      out coords = unique([b, floor(xyz / 2ts) 2ts]) sorted by (b, x, y, z), out stride 2ts,
                                                                         y[c'] = sum_o x[c' + ts o] W[kidx(o)]
  * transposed, k = 3:    from a coarse set at 2ts onto a GIVEN fine set at ts,
                                                                         y[c]  = sum_o x[c  - ts o] W[kidx(o)]
Offsets never cross batch indices.  The offset numbering and the sorted output order are this project's choice (MinkowskiEngine
cannot be imported on this platform): parity unpinned against MinkowskiEngine's own checkpoints.

``build_kernel_map`` turns the coordinates into the two int32 tables the kernels read.  One map serves every layer at its level:
build it once per batch and pass it in.  Two backends give the same integers: ``"torch"`` (the default; plumbing: a sort and
``searchsorted`` per offset in torch, device or CPU tensors alike) and ``"hip"`` (device tensors only: the packing, the coarser keys
and one lookup kernel per table of include/csn_hip.h section 17 around ``torch.sort`` / ``torch.unique``);
``tuning.override(native_kernel_maps=True)`` makes ``"hip"`` what ``backend=None`` means for device tensors.
``sparse_conv3d`` is one autograd node on ``csn_sparse_conv_fwd_f32`` / ``csn_sparse_conv_bwd_f32`` (include/csn_hip.h section
14); ``SparseConv3d`` / ``SparseConvTranspose3d`` hold MinkowskiEngine's ``kernel`` parameter; ``SparseBasicBlock`` is the
residual block with the reference's attribute names (its batch norms are ``nn.BatchNorm1d`` through ATen).

The kernel-2 stride-2 convolution and its transposed form (MinkowskiNet/models/res16unet.py: ``conv*s2`` / ``convtr*s2``) stand
beside that surface: kernel 2 at stride 2 partitions the fine voxels, so ``build_octant_map`` keeps one parent and one octant per
fine row instead of a table, and ``octant_conv_down`` / ``octant_conv_up`` (``SparseConvDown2`` / ``SparseConvUp2``) are one
autograd node each on ``csn_octant_*`` (include/csn_hip.h section 21).  ``build_octant_map`` has the two backends of
``build_kernel_map``: torch ops, or the partition and the stable counting sort of section 22 around ``torch.sort`` /
``torch.unique``.  ``cat_conv3d`` is a convolution on a concatenation that is never formed.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as CF
from . import tuning

_NO_CPU = "csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path"
BACKENDS = ("torch", "hip")
_B_BITS, _C_BITS = 15, 16
_C_BIAS = 1 << (_C_BITS - 1)


def _pack(coords: torch.Tensor) -> torch.Tensor:
    """[b, x, y, z] -> one int64 key whose order is the lexicographic order of (b, x, y, z)."""
    c = coords.long()
    return (c[:, 0] << (3 * _C_BITS)) | ((c[:, 1] + _C_BIAS) << (2 * _C_BITS)) | ((c[:, 2] + _C_BIAS) << _C_BITS) | (c[:, 3] + _C_BIAS)


def _unpack(keys: torch.Tensor) -> torch.Tensor:
    m = (1 << _C_BITS) - 1
    return torch.stack([keys >> (3 * _C_BITS), ((keys >> (2 * _C_BITS)) & m) - _C_BIAS, ((keys >> _C_BITS) & m) - _C_BIAS,
                        (keys & m) - _C_BIAS], dim=1)


def _check_shape(coords: torch.Tensor, what: str) -> None:
    if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < 1 or coords.dtype.is_floating_point:
        raise ValueError(f"{what} must be a non-empty (n, 4) integer tensor [b, x, y, z]")


def _check_coords(coords: torch.Tensor, ts: int, what: str) -> torch.Tensor:
    _check_shape(coords, what)
    c = coords.long()
    if int(c[:, 0].min()) < 0 or int(c[:, 0].max()) >= (1 << _B_BITS):
        raise ValueError(f"{what}: batch indices must lie in [0, {1 << _B_BITS})")
    if int(c[:, 1:].min()) < -_C_BIAS or int(c[:, 1:].max()) >= _C_BIAS:
        raise ValueError(f"{what}: x, y, z must lie in [{-_C_BIAS}, {_C_BIAS})")
    if bool((c[:, 1:] % ts != 0).any()):
        raise ValueError(f"{what}: x, y, z must be multiples of the tensor stride {ts}")
    return c


class _Index:
    """Sorted keys of a coordinate set: row lookup by coordinates."""

    def __init__(self, coords: torch.Tensor, what: str):
        self.keys, self.perm = torch.sort(_pack(coords))
        if bool((self.keys[1:] == self.keys[:-1]).any()):
            raise ValueError(f"{what} holds duplicate rows")

    def rows(self, coords: torch.Tensor) -> torch.Tensor:
        """int32 row of every coordinate, -1 where the set has none (or the coordinate leaves the packed range)."""
        ok = ((coords[:, 1:] >= -_C_BIAS) & (coords[:, 1:] < _C_BIAS)).all(dim=1)
        q = _pack(coords.clamp(min=-_C_BIAS, max=_C_BIAS - 1))
        pos = torch.searchsorted(self.keys, q).clamp_(max=self.keys.numel() - 1)
        hit = ok & (self.keys[pos] == q)
        return torch.where(hit, self.perm[pos], torch.full_like(pos, -1)).int()


def kernel_offsets(kernel_size: int, device=None) -> torch.Tensor:
    """(KV, 3) offsets (ox, oy, oz) in kidx order: x fastest."""
    r = kernel_size // 2
    a = torch.arange(-r, r + 1, device=device)
    oz, oy, ox = torch.meshgrid(a, a, a, indexing="ij")
    return torch.stack([ox.reshape(-1), oy.reshape(-1), oz.reshape(-1)], dim=1)


class KernelMap:
    """The tables of one convolution geometry between two coordinate sets.

    ``fwd (KV, n_out)`` int32: the input row that feeds output row j at offset k, or -1; ``bwd (KV, n_in)`` int32: the output row
    that input row i feeds at offset k, or -1.  At stride 1 ``bwd[k] = fwd[KV - 1 - k]``: no second table is searched or kept —
    ``bwd_table`` is None there, which the backward kernel takes as "walk ``fwd`` in reversed offset order"; ``bwd`` forms the
    reversed copy for whoever wants to look at it (torch has no negative-stride view) and does not keep it.
    ``transpose()`` is the map of the opposite direction over the same tables."""

    def __init__(self, in_coords, out_coords, kernel_size, stride, in_tensor_stride, out_tensor_stride, transposed, fwd, bwd):
        self.in_coords, self.out_coords = in_coords, out_coords
        self.kernel_size, self.stride = kernel_size, stride
        self.in_tensor_stride, self.out_tensor_stride = in_tensor_stride, out_tensor_stride
        self.transposed = transposed
        self.fwd = fwd
        self.bwd_table = bwd                                           # None: the stride-1 identity on ``fwd``

    @property
    def bwd(self) -> torch.Tensor:
        return self.fwd.flip(0) if self.bwd_table is None else self.bwd_table

    @property
    def KV(self) -> int:
        return self.kernel_size ** 3

    @property
    def n_in(self) -> int:
        return self.in_coords.shape[0]

    @property
    def n_out(self) -> int:
        return self.out_coords.shape[0]

    def transpose(self) -> "KernelMap":
        """The map from ``out_coords`` back onto ``in_coords``: a stride-2 map becomes the transposed convolution's map (and the
        other way round), sharing the tables.  A stride-1 map is its own transpose with the offsets reversed."""
        if self.stride == 1:
            return KernelMap(self.out_coords, self.in_coords, self.kernel_size, 1, self.out_tensor_stride, self.in_tensor_stride,
                             False, self.bwd, None if self.bwd_table is None else self.fwd)
        return KernelMap(self.out_coords, self.in_coords, self.kernel_size, self.stride, self.out_tensor_stride,
                         self.in_tensor_stride, not self.transposed, self.bwd, self.fwd)

    def to(self, device) -> "KernelMap":
        mv = lambda t: None if t is None else t.to(device)
        return KernelMap(mv(self.in_coords), mv(self.out_coords), self.kernel_size, self.stride, self.in_tensor_stride,
                         self.out_tensor_stride, self.transposed, mv(self.fwd), mv(self.bwd_table))


def build_kernel_map(coords: torch.Tensor, kernel_size: int = 3, stride: int = 1, tensor_stride: int = 1,
                     out_coords: Optional[torch.Tensor] = None, transposed: bool = False, backend: Optional[str] = None) -> KernelMap:
    """The kernel map of one convolution geometry (module docstring).  ``coords`` are the input rows' coordinates at
    ``tensor_stride``.  ``stride == 2`` generates the coarser coordinates unless ``out_coords`` gives them; ``transposed`` goes from
    ``coords`` (coarse, at ``tensor_stride``) onto the given ``out_coords`` at ``tensor_stride // 2``.

    ``backend``: ``"torch"`` builds the tables with torch ops (device or CPU tensors); ``"hip"`` with the kernels of include/csn_hip.h
    section 17 — device tensors only (``CsnError`` otherwise), the same attributes, dtypes and integers, the same ``ValueError``
    messages (raised after the launches: one status word is read back per call).  None takes ``"hip"`` for device tensors when
    ``tuning.current().native_kernel_maps`` is set and ``"torch"`` otherwise; any other value raises ``ValueError``."""
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size {kernel_size} is not supported: odd sizes only")
    if kernel_size not in (1, 3, 5):
        raise ValueError(f"kernel_size {kernel_size} is not supported: the kernels take 1, 3 and 5")
    if stride not in (1, 2):
        raise ValueError(f"stride {stride} is not supported: 1 or 2")
    if stride == 2 and kernel_size != 3:
        raise ValueError("stride 2 takes kernel_size 3 only")
    if transposed and stride != 2:
        raise ValueError("the transposed convolution is the kernel-3 stride-2 one")
    if transposed and out_coords is None:
        raise ValueError("the transposed convolution goes onto a given coordinate set: pass out_coords (coordinates are not generated)")
    if tensor_stride < 1 or (transposed and tensor_stride % 2):
        raise ValueError(f"tensor_stride {tensor_stride} is not valid here")
    backend = resolve_backend(backend, coords, out_coords)
    if transposed:
        ts, out_ts = tensor_stride // 2, tensor_stride // 2        # ts: the step of the offsets (the finer of the two strides)
    else:
        ts, out_ts = tensor_stride, tensor_stride * stride
    if backend == "hip":
        if out_coords is not None and out_coords.device != coords.device:
            raise ValueError("coords and out_coords must be on one device")
        return _build_kernel_map_hip(coords, kernel_size, stride, tensor_stride, out_coords, transposed, ts, out_ts)
    c_in = _check_coords(coords, tensor_stride, "coords")
    idx_in = _Index(c_in, "coords")
    if out_coords is not None:
        if out_coords.device != coords.device:
            raise ValueError("coords and out_coords must be on one device")
        c_out = _check_coords(out_coords, out_ts, "out_coords")
        idx_out = _Index(c_out, "out_coords")
    elif stride == 1:
        c_out, idx_out = c_in, idx_in
    else:
        down = c_in.clone()
        down[:, 1:] = torch.div(c_in[:, 1:], out_ts, rounding_mode="floor") * out_ts      # floor, not truncation, for negatives
        c_out = _unpack(torch.unique(_pack(down), sorted=True))
        idx_out = _Index(c_out, "out_coords")
    off = kernel_offsets(kernel_size, coords.device) * ts
    sign = -1 if transposed else 1

    def table(index, at, s):
        rows = []
        for o in off:
            q = at.clone()
            q[:, 1:] += s * o
            rows.append(index.rows(q))
        return torch.stack(rows).contiguous()

    fwd = table(idx_in, c_out, sign)
    bwd = None if (stride == 1 and out_coords is None) else table(idx_out, c_in, -sign)
    return KernelMap(c_in, c_out, kernel_size, stride, tensor_stride, out_ts, transposed, fwd, bwd)


# ------------------------------------------------------------------------------------------------------
# the native backend (include/csn_hip.h section 17)
# ------------------------------------------------------------------------------------------------------
def resolve_backend(backend: Optional[str], *tensors: Optional[torch.Tensor]) -> str:
    """``"torch"`` or ``"hip"`` for a call on ``tensors``.  None follows ``tuning.current().native_kernel_maps`` for device tensors;
    CPU tensors keep the torch backend under the switch and raise ``CsnError`` where ``"hip"`` is asked for by name."""
    if backend is not None and backend not in BACKENDS:
        raise ValueError(f"backend {backend!r} is not known: one of {BACKENDS}, or None for the tuning switch")
    on_device = all(t.is_cuda for t in tensors if t is not None)
    if backend is None:
        return "hip" if tuning.current().native_kernel_maps and on_device else "torch"
    if backend == "hip" and not on_device:
        raise _lib.CsnError(_NO_CPU)
    return backend


class _KeySet:
    """A coordinate set for the native lookups: ``coords (n, 4)`` int64, ``keys (n,)`` in row order, ``sorted (n,)`` ascending,
    ``rows (n,)`` int32 the row of every sorted key — None where the rows are in key order already."""

    def __init__(self, coords, keys, sorted_keys, rows):
        self.coords, self.keys, self.sorted, self.rows = coords, keys, sorted_keys, rows


def _new_status(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def _read_status(status: torch.Tensor) -> int:
    """The one host read of a native build."""
    return int(status.item())


def _coord_keys(c: torch.Tensor, ts: int, status: torch.Tensor) -> torch.Tensor:
    """(17a): the packed keys of ``c (n, 4)`` int64; range and tensor-stride failures go into ``status``."""
    cc = c.contiguous()
    keys = torch.empty(cc.shape[0], dtype=torch.int64, device=cc.device)
    _lib.check(_lib.lib().csn_coord_keys_i64(CF._ptr(cc), cc.shape[0], ts, CF._ptr(keys), CF._ptr(status), CF._stream()),
               "csn_coord_keys_i64")
    return keys


def _key_set(coords: torch.Tensor, ts: int, what: str, status: torch.Tensor) -> _KeySet:
    """(17a) and one sort: what ``_check_coords`` + ``_Index`` are to the torch backend."""
    _check_shape(coords, what)
    c = coords.long()
    keys = _coord_keys(c, ts, status)
    skeys, perm = torch.sort(keys)
    return _KeySet(c, keys, skeys, perm.int())


def _coarse_set(fine: _KeySet, out_ts: int) -> _KeySet:
    """(17b), then the sorted unique keys: the coarser level of ``fine``, its rows in key order."""
    down = torch.empty_like(fine.keys)
    n = down.numel()
    _lib.check(_lib.lib().csn_coord_down_i64(CF._ptr(fine.keys), n, out_ts, CF._ptr(down), CF._stream()), "csn_coord_down_i64")
    uniq = torch.unique(down, sorted=True)
    return _KeySet(_unpack(uniq), uniq, uniq, None)


def _lookup(where: _KeySet, at: _KeySet, kernel_size: int, step: int, status: torch.Tensor) -> torch.Tensor:
    """(17c): ``table (KV, n_at)`` int32, the row in ``where`` of "row j of ``at`` + step * offset", or -1; a set that is not
    strictly ascending (a duplicate row) goes into ``status``."""
    n_set, n_query = where.sorted.numel(), at.keys.numel()
    table = torch.empty((kernel_size ** 3, n_query), dtype=torch.int32, device=at.keys.device)
    _lib.check(_lib.lib().csn_kernel_map_i32(CF._ptr(where.sorted), CF._ptr(where.rows), n_set, CF._ptr(at.keys), n_query, kernel_size,
                                             step, CF._ptr(table), CF._ptr(status), CF._stream()), "csn_kernel_map_i32")
    return table


def _raise_for_status(word: int, sets) -> None:
    """A non-zero status word of a native build.  The word says THAT a set is bad; which one, and the torch backend's own message for
    it, come from that backend's checks on ``sets`` = [(coords, tensor stride, name)] in its order (the failing call's price)."""
    if word == 0:
        return
    for coords, ts, what in sets:
        _Index(_check_coords(coords, ts, what), what)
    raise ValueError(f"the coordinates are not valid (kernel-map status {word})")


def _build_kernel_map_hip(coords, kernel_size, stride, tensor_stride, out_coords, transposed, ts, out_ts) -> KernelMap:
    status = _new_status(coords.device)
    s_in = _key_set(coords, tensor_stride, "coords", status)
    sets = [(coords, tensor_stride, "coords")]
    if out_coords is not None:
        s_out = _key_set(out_coords, out_ts, "out_coords", status)
        sets.append((out_coords, out_ts, "out_coords"))
    elif stride == 1:
        s_out = s_in
    else:
        s_out = _coarse_set(s_in, out_ts)
    step = -ts if transposed else ts
    fwd = _lookup(s_in, s_out, kernel_size, step, status)
    bwd = None if (stride == 1 and out_coords is None) else _lookup(s_out, s_in, kernel_size, -step, status)
    _raise_for_status(_read_status(status), sets)
    return KernelMap(s_in.coords, s_out.coords, kernel_size, stride, tensor_stride, out_ts, transposed, fwd, bwd)


# ------------------------------------------------------------------------------------------------------
# the autograd node
# ------------------------------------------------------------------------------------------------------
class _SparseConv(torch.autograd.Function):
    """y = gather-GEMM(x, kmap.fwd, w) + b through ``csn_sparse_conv_fwd_f32`` / ``csn_sparse_conv_bwd_f32``."""

    @staticmethod
    def forward(ctx, x, w, b, kmap):
        CF._need_cuda(x, w, b, kmap.fwd)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        ctx.rows16 = tuning.current().rows_single_product
        x = x.contiguous()
        w_c = w.detach().contiguous()
        b_c = None if b is None else b.detach().reshape(-1).contiguous()
        KV, c_in, c_out = w_c.shape
        n_in, n_out = kmap.n_in, kmap.n_out
        y = torch.empty((n_out, c_out), device=x.device, dtype=torch.float32)
        with CF.rows16(ctx.rows16):
            _lib.check(L.csn_sparse_conv_fwd_f32(CF._ptr(x), c_in, n_in, CF._ptr(kmap.fwd), n_out, KV, c_in, c_out, CF._ptr(w_c),
                                                 CF._ptr(b_c), CF._ptr(y), c_out, CF._stream()), "csn_sparse_conv_fwd_f32")
        ctx.save_for_backward(x, w_c)
        ctx.kmap = kmap
        ctx.b_shape = None if b is None else b.shape
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        with CF.math_mode(CF.backward_mode(ctx.mode)), CF.rows16(ctx.rows16):
            x, w = ctx.saved_tensors
            need_b = ctx.b_shape is not None and ctx.needs_input_grad[2]
            dx, dw, db = _sparse_conv_backward(dy, x, x.shape[1], w, ctx.kmap, ctx.needs_input_grad[0], ctx.needs_input_grad[1], need_b)
            return dx, dw, None if db is None else db.reshape(ctx.b_shape), None


def _workspace(n_bytes: int, device) -> torch.Tensor:
    """The scratch tensor of one call: the library's byte count, never fewer than 16 (a pointer the checks take)."""
    return torch.empty((max(n_bytes, 16),), device=device, dtype=torch.uint8)


def _sparse_conv_backward(dz, x, ld_x, w, kmap, need_x, need_w, need_b=False):
    """``(dx, dw, dbias)`` of the convolution ``kmap`` describes, each None unless wanted — the backward of every node on a kernel
    map.  ``x (n_in, c_in)`` is the saved input with its row pitch ``ld_x`` in elements: fp32 rows go to ``csn_sparse_conv_bwd_f32``,
    bf16 rows to ``csn_sparse_conv_bwd_t16``, which takes nothing else.  ``w (KV, c_in, c_out)`` may be None without dx.  The caller
    holds its node's math-mode and rows16 brackets."""
    if not (need_x or need_w or need_b):
        return None, None, None
    L = _lib.lib()
    KV, n_in, n_out = kmap.KV, kmap.n_in, kmap.n_out
    c_in, c_out = x.shape[1], dz.shape[1]
    dz = dz.contiguous()
    dx = dz.new_empty((n_in, c_in)) if need_x else None                     # fp32 on dz's device, whatever x is
    dw = dz.new_empty((KV, c_in, c_out)) if need_w else None
    db = dz.new_empty((c_out,)) if need_b else None
    ws_n = int(L.csn_sparse_conv_workspace_bytes(n_in, n_out, KV, c_in, c_out, 1))
    ws = _workspace(ws_n, dz.device)
    bwd = kmap.bwd_table if need_x else None                                # None at stride 1: the kernel reverses ``fwd``
    tail = (ld_x, n_in, n_out, KV, c_in, c_out, CF._ptr(kmap.fwd), CF._ptr(bwd), CF._ptr(w), CF._ptr(dx), c_in, CF._ptr(dw), CF._ptr(db),
            CF._ptr(ws), ws_n, CF._stream())
    if x.dtype == torch.bfloat16:
        _lib.check(L.csn_sparse_conv_bwd_t16(CF._ptr(dz), c_out, CF._ptr(x), 1, *tail), "csn_sparse_conv_bwd_t16")
    else:
        _lib.check(L.csn_sparse_conv_bwd_f32(CF._ptr(dz), c_out, CF._ptr(x), *tail), "csn_sparse_conv_bwd_f32")
    return dx, dw, db


def sparse_conv3d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], kmap: KernelMap) -> torch.Tensor:
    """``y (n_out, c_out)`` of the convolution ``kmap`` describes: ``x (n_in, c_in)``, ``weight (KV, c_in, c_out)``, ``bias``
    ``(c_out,)`` / ``(1, c_out)`` or None.  An input width that is not a multiple of 32 (the stem's 3 colour channels) is
    zero-padded to one, rows and weight alike; autograd slices the gradients back."""
    if not (x.is_cuda and weight.is_cuda):
        raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1]:
        raise ValueError("x must be (n_in, c_in) and weight (KV, c_in, c_out)")
    if weight.shape[0] != kmap.KV:
        raise ValueError(f"the weight holds {weight.shape[0]} offsets, the map {kmap.KV}")
    if x.shape[0] != kmap.n_in:
        raise ValueError(f"x has {x.shape[0]} rows, the map's input set {kmap.n_in}")
    c_in, c_out = weight.shape[1], weight.shape[2]
    if c_out % 32 or not 32 <= c_out <= 256:
        raise ValueError(f"c_out {c_out} is not supported: a multiple of 32 in [32, 256]")
    if bias is not None and bias.numel() != c_out:
        raise ValueError(f"bias must hold {c_out} values")
    pad = -c_in % 32
    if c_in + pad > 256:
        raise ValueError(f"c_in {c_in} is not supported: at most 256")
    if pad:
        x = F.pad(x, (0, pad))
        weight = F.pad(weight, (0, 0, 0, pad))
    return _SparseConv.apply(x.float(), weight, bias, kmap)


def cat_conv3d(parts, weight: torch.Tensor, kmap: KernelMap) -> torch.Tensor:
    """The convolution of ``torch.cat(parts, dim=1)`` as the sum of the convolutions of the parts: ``parts`` is a list of ``(n, c_p)``
    maps and ``weight (KV, sum c_p, c_out)`` ONE kernel.  The concatenation is never formed and every part (<= 256 wide) is taken
    by the existing kernels, so a decoder block may be wider than 256 at its input.  Autograd composes the gradient."""
    if not parts:
        raise ValueError("cat_conv3d needs at least one part")
    if weight.dim() != 3 or sum(int(p.shape[1]) for p in parts) != weight.shape[1]:
        raise ValueError("the parts' widths must add up to the weight's c_in")
    y, c0 = None, 0
    for part in parts:
        c1 = c0 + int(part.shape[1])
        t = sparse_conv3d(part, weight[:, c0:c1], None, kmap)
        y = t if y is None else y + t
        c0 = c1
    return y


# ------------------------------------------------------------------------------------------------------
# kernel 2 at stride 2: the octant map and its two convolutions (include/csn_hip.h section 21)
# ------------------------------------------------------------------------------------------------------
class OctantMap:
    """The partition of a fine coordinate set at ``ts`` by its coarse set at ``2 ts`` (all index tensors int32):

    ``parent (n_fine,)`` the coarse row of every fine row; ``octant (n_fine,)`` = ox + 2 oy + 4 oz with o = (xyz - floor(xyz /
    2ts) 2ts) / ts in {0, 1}^3 (x fastest, as in ``kidx``); ``children (8, n_coarse)`` the fine row in octant k of coarse row j, or
    -1; ``order (n_fine,)`` the fine rows sorted by (octant, row) and ``seg (9,)`` its segment bounds, on the device like the
    rest.  The octant numbering is this project's choice, like the offset numbering: parity unpinned against MinkowskiEngine's own
    checkpoints."""

    def __init__(self, in_coords, out_coords, in_tensor_stride, out_tensor_stride, parent, octant, children, order, seg):
        self.in_coords, self.out_coords = in_coords, out_coords
        self.in_tensor_stride, self.out_tensor_stride = in_tensor_stride, out_tensor_stride
        self.parent, self.octant, self.children, self.order, self.seg = parent, octant, children, order, seg

    @property
    def n_fine(self) -> int:
        return self.in_coords.shape[0]

    @property
    def n_coarse(self) -> int:
        return self.out_coords.shape[0]

    def to(self, device) -> "OctantMap":
        mv = lambda t: t.to(device)
        return OctantMap(mv(self.in_coords), mv(self.out_coords), self.in_tensor_stride, self.out_tensor_stride, mv(self.parent),
                         mv(self.octant), mv(self.children), mv(self.order), mv(self.seg))


OCTANT_ORDER_TILE, OCTANT_ORDER_SCAN = 256, 256     # csrc/csn_kernels.h: rows per tile of (22b), tiles per pass of its scan
_NO_PARENT = "out_coords misses the parent of some row of coords"


def _octant_map(fine: _KeySet, coarse: _KeySet, ts: int, status: torch.Tensor, check_fine: bool) -> OctantMap:
    """(22a) and (22b): the octant map of ``fine`` at ``ts`` onto ``coarse``.  ``check_fine`` hands the sorted fine keys in for the
    duplicate check; a caller whose (17c) lookup on ``fine`` has made it passes False."""
    L = _lib.lib()
    dev = fine.keys.device
    n_fine, n_coarse = fine.keys.numel(), coarse.sorted.numel()
    parent = torch.empty(n_fine, dtype=torch.int32, device=dev)
    octant = torch.empty(n_fine, dtype=torch.int32, device=dev)
    children = torch.empty((8, n_coarse), dtype=torch.int32, device=dev)
    _lib.check(L.csn_octant_partition_i32(CF._ptr(fine.keys), CF._ptr(fine.sorted) if check_fine else None, n_fine, ts,
                                          CF._ptr(coarse.sorted), CF._ptr(coarse.rows), n_coarse, CF._ptr(parent), CF._ptr(octant),
                                          CF._ptr(children), CF._ptr(status), CF._stream()), "csn_octant_partition_i32")
    order = torch.empty(n_fine, dtype=torch.int32, device=dev)
    seg = torch.empty(9, dtype=torch.int32, device=dev)
    ws_n = int(L.csn_octant_order_workspace_bytes(n_fine))
    ws = torch.empty(ws_n // 4, dtype=torch.int32, device=dev)
    _lib.check(L.csn_octant_order_i32(CF._ptr(octant), n_fine, CF._ptr(order), CF._ptr(seg), CF._ptr(ws), ws_n, CF._ptr(status),
                                      CF._stream()), "csn_octant_order_i32")
    return OctantMap(fine.coords, coarse.coords, ts, 2 * ts, parent, octant, children, order, seg)


def _build_octant_map_hip(coords, ts, out_coords) -> OctantMap:
    status = _new_status(coords.device)
    s_in = _key_set(coords, ts, "coords", status)
    sets = [(coords, ts, "coords")]
    if out_coords is not None:
        s_out = _key_set(out_coords, 2 * ts, "out_coords", status)
        sets.append((out_coords, 2 * ts, "out_coords"))
    else:
        s_out = _coarse_set(s_in, 2 * ts)
    omap = _octant_map(s_in, s_out, ts, status, True)
    word = _read_status(status)
    if word & 16:                                                    # the sets' own failures first, in the torch backend's order
        _raise_for_status(word & ~16, sets)
        raise ValueError(_NO_PARENT)
    _raise_for_status(word, sets)
    return omap


def build_octant_map(coords: torch.Tensor, tensor_stride: int = 1, out_coords: Optional[torch.Tensor] = None,
                     backend: Optional[str] = None) -> OctantMap:
    """The octant map of ``coords (n_fine, 4) = [b, x, y, z]`` (unique rows in any order, multiples of ``tensor_stride``) onto the
    coarse set ``build_kernel_map(..., stride=2)`` generates — ``unique([b, floor(xyz / 2ts) 2ts])`` sorted by (b, x, y, z) — or
    onto ``out_coords`` when given (it must hold every parent: ``ValueError``).  The octant numbering is this project's choice,
    unpinned against MinkowskiEngine (``OctantMap``).

    ``backend`` as in ``build_kernel_map``.  ``"torch"``: torch ops on the coordinates' device (one ``searchsorted``, one stable
    sort, one scatter), with a host read per check.  ``"hip"``: the kernels of include/csn_hip.h section 22 around ``torch.sort`` /
    ``torch.unique`` — device tensors only (``CsnError`` otherwise), the same attributes, dtypes and integers, the same
    ``ValueError`` messages (raised after the launches: one status word is read back per call).  None takes ``"hip"`` for device
    tensors when ``tuning.current().native_kernel_maps`` is set and ``"torch"`` otherwise."""
    ts = int(tensor_stride)
    if ts < 1:
        raise ValueError(f"tensor_stride {tensor_stride} is not valid here")
    out_ts = 2 * ts
    if resolve_backend(backend, coords, out_coords) == "hip":
        if out_coords is not None and out_coords.device != coords.device:
            raise ValueError("coords and out_coords must be on one device")
        return _build_octant_map_hip(coords, ts, out_coords)
    c_in = _check_coords(coords, ts, "coords")
    _Index(c_in, "coords")                                           # duplicates
    down = c_in.clone()
    down[:, 1:] = torch.div(c_in[:, 1:], out_ts, rounding_mode="floor") * out_ts          # floor, not truncation, for negatives
    if out_coords is not None:
        if out_coords.device != coords.device:
            raise ValueError("coords and out_coords must be on one device")
        c_out = _check_coords(out_coords, out_ts, "out_coords")
        idx_out = _Index(c_out, "out_coords")
    else:
        c_out = _unpack(torch.unique(_pack(down), sorted=True))
        idx_out = _Index(c_out, "out_coords")
    parent = idx_out.rows(down)
    if out_coords is not None and bool((parent < 0).any()):
        raise ValueError(_NO_PARENT)
    o = (c_in[:, 1:] - down[:, 1:]) // ts
    octant = (o[:, 0] + 2 * o[:, 1] + 4 * o[:, 2]).int()
    n_fine, n_coarse = c_in.shape[0], c_out.shape[0]
    rows = torch.arange(n_fine, device=coords.device, dtype=torch.int32)
    children = torch.full((8 * n_coarse,), -1, dtype=torch.int32, device=coords.device)
    children[octant.long() * n_coarse + parent.long()] = rows
    order = torch.sort(octant, stable=True)[1].int()
    seg = torch.zeros(9, dtype=torch.int32, device=coords.device)
    seg[1:] = torch.cumsum(torch.bincount(octant, minlength=8), 0).int()
    return OctantMap(c_in, c_out, ts, out_ts, parent, octant, children.view(8, n_coarse), order, seg)


class _OctantConv(torch.autograd.Function):
    """``up`` False: y[j] = sum_k x[children[k][j]] W[k] + b;  True: y[i] = x[parent[i]] W[octant[i]] + b — one node on
    ``csn_octant_{down,up}_fwd_f32`` / ``_bwd_f32``."""

    @staticmethod
    def forward(ctx, x, w, b, omap, up):
        CF._need_cuda(x, w, b, omap.parent)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        x = x.contiguous()
        w_c = w.detach().contiguous()
        b_c = None if b is None else b.detach().reshape(-1).contiguous()
        _, c_in, c_out = w_c.shape
        n_fine, n_coarse = omap.n_fine, omap.n_coarse
        y = torch.empty((n_fine if up else n_coarse, c_out), device=x.device, dtype=torch.float32)
        if up:
            _lib.check(L.csn_octant_up_fwd_f32(CF._ptr(x), c_in, n_coarse, CF._ptr(omap.parent), CF._ptr(omap.order), CF._ptr(omap.seg),
                                               n_fine, c_in, c_out, CF._ptr(w_c), CF._ptr(b_c), CF._ptr(y), c_out, CF._stream()),
                       "csn_octant_up_fwd_f32")
        else:
            _lib.check(L.csn_octant_down_fwd_f32(CF._ptr(x), c_in, n_fine, CF._ptr(omap.children), n_coarse, c_in, c_out, CF._ptr(w_c),
                                                 CF._ptr(b_c), CF._ptr(y), c_out, CF._stream()), "csn_octant_down_fwd_f32")
        ctx.save_for_backward(x, w_c)
        ctx.omap, ctx.up = omap, up
        ctx.b_shape = None if b is None else b.shape
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        with CF.math_mode(CF.backward_mode(ctx.mode)):
            x, w = ctx.saved_tensors
            need_b = ctx.b_shape is not None and ctx.needs_input_grad[2]
            dx, dw, db = _octant_conv_backward(dy, x, w, ctx.omap, ctx.up, ctx.needs_input_grad[0], ctx.needs_input_grad[1], need_b)
            return dx, dw, None if db is None else db.reshape(ctx.b_shape), None, None


def _octant_conv_backward(dz, x, w, omap, up, need_x, need_w, need_b=False):
    """``(dx, dw, dbias)`` of an octant convolution that saved contiguous ``(x, w)``, each None unless wanted:
    ``csn_octant_{down,up}_bwd_f32``.  The caller holds its node's math-mode bracket."""
    if not (need_x or need_w or need_b):
        return None, None, None
    L = _lib.lib()
    _, c_in, c_out = w.shape
    n_fine, n_coarse = omap.n_fine, omap.n_coarse
    dz = dz.contiguous()
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty_like(w) if need_w else None
    db = torch.empty((c_out,), device=x.device, dtype=torch.float32) if need_b else None
    ws_n = int(L.csn_octant_conv_workspace_bytes(n_fine, n_coarse, c_in, c_out, int(up), 1))
    ws = _workspace(ws_n, x.device)
    head = (CF._ptr(dz), c_out, CF._ptr(x), c_in, n_fine, n_coarse, c_in, c_out)
    tail = (CF._ptr(omap.parent), CF._ptr(omap.order), CF._ptr(omap.seg), CF._ptr(w), CF._ptr(dx), c_in, CF._ptr(dw), CF._ptr(db),
            CF._ptr(ws), ws_n, CF._stream())
    if up:
        _lib.check(L.csn_octant_up_bwd_f32(*head, CF._ptr(omap.children), *tail), "csn_octant_up_bwd_f32")
    else:
        _lib.check(L.csn_octant_down_bwd_f32(*head, *tail), "csn_octant_down_bwd_f32")
    return dx, dw, db


def _octant_conv(x, weight, bias, omap, up):
    if not (x.is_cuda and weight.is_cuda):
        raise _lib.CsnError(_NO_CPU)
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1]:
        raise ValueError("x must be (n_in, c_in) and weight (8, c_in, c_out)")
    if weight.shape[0] != 8:
        raise ValueError(f"the weight holds {weight.shape[0]} offsets, the octant map 8")
    n_in = omap.n_coarse if up else omap.n_fine
    if x.shape[0] != n_in:
        raise ValueError(f"x has {x.shape[0]} rows, the map's input set {n_in}")
    c_in, c_out = weight.shape[1], weight.shape[2]
    for name, c in (("c_in", c_in), ("c_out", c_out)):
        if c % 32 or not 32 <= c <= 256:
            raise ValueError(f"{name} {c} is not supported: a multiple of 32 in [32, 256]")
    if bias is not None and bias.numel() != c_out:
        raise ValueError(f"bias must hold {c_out} values")
    return _OctantConv.apply(x.float(), weight, bias, omap, up)


def octant_conv_down(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], omap: OctantMap) -> torch.Tensor:
    """The kernel-2 stride-2 convolution: ``x (n_fine, c_in)`` -> ``(n_coarse, c_out)``, ``y[j] = sum_k x[children[k][j]] W[k] + b``;
    ``weight (8, c_in, c_out)``, widths multiples of 32 in [32, 256]."""
    return _octant_conv(x, weight, bias, omap, False)


def octant_conv_up(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], omap: OctantMap) -> torch.Tensor:
    """Its transposed form, back onto the map's fine set: ``x (n_coarse, c_in)`` -> ``(n_fine, c_out)``,
    ``y[i] = x[parent[i]] W[octant[i]] + b`` — one weight per row."""
    return _octant_conv(x, weight, bias, omap, True)


# ------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------
class SparseConv3d(nn.Module):
    """``ME.MinkowskiConvolution(c_in, c_out, kernel_size, stride, dimension=3)`` on rows and a kernel map: parameter ``kernel``
    ``(KV, c_in, c_out)`` and, when asked, ``bias (1, c_out)`` — MinkowskiEngine's names and shapes."""

    transposed = False

    def __init__(self, c_in: int, c_out: int, kernel_size: int = 3, stride: int = 1, bias: bool = False):
        super().__init__()
        if kernel_size not in (1, 3, 5):
            raise ValueError(f"kernel_size {kernel_size} is not supported: 1, 3 or 5")
        if stride not in (1, 2) or (stride == 2 and kernel_size != 3):
            raise ValueError("stride 1, or stride 2 with kernel_size 3")
        if c_out % 32 or not 32 <= c_out <= 256 or not 1 <= c_in <= 256:
            raise ValueError("widths: c_out a multiple of 32 in [32, 256], c_in in [1, 256]")
        self.c_in, self.c_out, self.kernel_size, self.stride = c_in, c_out, kernel_size, stride
        KV = kernel_size ** 3
        self.kernel = nn.Parameter(torch.empty(KV, c_in, c_out))
        self.bias = nn.Parameter(torch.zeros(1, c_out)) if bias else None
        nn.init.normal_(self.kernel, std=(KV * c_in) ** -0.5)             # unit-variance outputs for unit-variance rows

    def forward(self, x: torch.Tensor, kmap: KernelMap) -> torch.Tensor:
        if kmap.kernel_size != self.kernel_size or kmap.stride != self.stride or kmap.transposed != self.transposed:
            raise ValueError(f"the map (kernel {kmap.kernel_size}, stride {kmap.stride}, transposed {kmap.transposed}) does not fit "
                             f"this layer (kernel {self.kernel_size}, stride {self.stride}, transposed {self.transposed})")
        return sparse_conv3d(x, self.kernel, self.bias, kmap)

    def extra_repr(self) -> str:
        return f"{self.c_in}, {self.c_out}, kernel_size={self.kernel_size}, stride={self.stride}, bias={self.bias is not None}"


class SparseConvTranspose3d(SparseConv3d):
    """``ME.MinkowskiConvolutionTranspose(c_in, c_out, kernel_size=3, stride=2, dimension=3)`` onto a given finer coordinate set:
    takes the ``transpose()`` of that level's stride-2 map (or a map built with ``transposed=True``)."""

    transposed = True

    def __init__(self, c_in: int, c_out: int, bias: bool = False):
        super().__init__(c_in, c_out, kernel_size=3, stride=2, bias=bias)


class SparseConvDown2(nn.Module):
    """``ME.MinkowskiConvolution(c_in, c_out, kernel_size=2, stride=2, dimension=3)`` on rows and an octant map: parameter
    ``kernel (8, c_in, c_out)`` and, when asked, ``bias (1, c_out)``."""

    up = False

    def __init__(self, c_in: int, c_out: int, bias: bool = False):
        super().__init__()
        if c_in % 32 or c_out % 32 or not 32 <= c_in <= 256 or not 32 <= c_out <= 256:
            raise ValueError("widths: c_in and c_out multiples of 32 in [32, 256]")
        self.c_in, self.c_out = c_in, c_out
        self.kernel = nn.Parameter(torch.empty(8, c_in, c_out))
        self.bias = nn.Parameter(torch.zeros(1, c_out)) if bias else None
        nn.init.normal_(self.kernel, std=(8 * c_in) ** -0.5)              # unit-variance outputs for unit-variance rows

    def forward(self, x: torch.Tensor, omap: OctantMap) -> torch.Tensor:
        if not isinstance(omap, OctantMap):
            raise ValueError(f"this layer (kernel 2, stride 2) takes an OctantMap, not {type(omap).__name__}")
        n_in = omap.n_coarse if self.up else omap.n_fine
        if x.shape[0] != n_in:
            raise ValueError(f"the map ({omap.n_fine} fine rows, {omap.n_coarse} coarse rows) does not fit the {x.shape[0]} rows "
                             f"given to this layer ({'transposed' if self.up else 'down'})")
        return _octant_conv(x, self.kernel, self.bias, omap, self.up)

    def extra_repr(self) -> str:
        return f"{self.c_in}, {self.c_out}, kernel_size=2, stride=2, bias={self.bias is not None}"


class SparseConvUp2(SparseConvDown2):
    """``ME.MinkowskiConvolutionTranspose(c_in, c_out, kernel_size=2, stride=2, dimension=3)`` back onto the fine set of the octant
    map that took the features down."""

    up = True


class SparseBasicBlock(nn.Module):
    """``BasicBlock`` of resnet_block.py:22-57: conv1 - norm1 - relu - conv2 - norm2, plus the residual (through ``downsample`` if
    given: a module of the rows), relu.  Both convolutions are kernel 3, stride 1 on the same map."""

    expansion = 1

    def __init__(self, inplanes: int, planes: int, bn_momentum: float = 0.02, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = SparseConv3d(inplanes, planes, kernel_size=3, stride=1)
        self.norm1 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.conv2 = SparseConv3d(planes, planes, kernel_size=3, stride=1)
        self.norm2 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.relu = nn.ReLU(inplace=False)
        self.downsample = downsample

    def forward(self, x: torch.Tensor, kmap: KernelMap) -> torch.Tensor:
        residual = x
        out = self.relu(self.norm1(self.conv1(x, kmap)))
        out = self.norm2(self.conv2(out, kmap))
        if self.downsample is not None:
            residual = self.downsample(x)
        return self.relu(out + residual)
