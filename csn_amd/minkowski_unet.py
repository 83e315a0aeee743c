"""MinkowskiNet's Res16UNet family on voxel rows, on the MI355X kernels.

Reference (marios2019/CSN):
  * ``Res16UNetBase`` and its classes                                  MinkowskiNet/models/res16unet.py:11-330
  * ``_make_layer`` (the blocks' ``downsample``)                        MinkowskiNet/models/resnet.py:86-127
  * ``BasicBlock``                                                      MinkowskiNet/models/modules/resnet_block.py:22-57

An encoder of four kernel-2 stride-2 convolutions, a decoder of four transposed ones, a list of ``BasicBlock`` after each and the
encoder's maps concatenated to the decoder's (``me.cat``).  The two resolution changes run on ``SparseConvDown2`` / ``SparseConvUp2``
over an ``OctantMap`` (include/csn_hip.h section 21), their BatchNorm through ATen.  The blocks run on the fused nodes of
minkowski_hrnet.py (``conv_stats`` + ``bn_act``, section 15): a block whose width changes has a ``downsample`` (kernel-1 convolution
+ BatchNorm) and sums TWO terms, ``norm2(conv2)`` and ``norm(downsample)``, in one ``bn_act`` launch.  A decoder block's input is
``[up | skip]``: up to 256 columns it is formed with ``torch.cat`` and takes the fused path; beyond, ``conv1`` and the ``downsample``
convolution go through ``cat_conv3d`` (the concatenation is never formed) with an ATen BatchNorm, and the rest of the block stays
fused.  ``fused=False`` runs everything on ``sparse_conv3d`` / the octant nodes + ATen: the timing baseline and the tests' yardstick.
``tuning.override(unet_fused_tail=True)`` (a fused network in training mode, opt-in) puts those two remaining layer kinds on the
fused nodes as well: a resolution change is ``octant_conv_stats`` + ``bn_act`` (section 26), ``conv1`` / ``downsample.0`` of a block
wider than 256 columns are ``cat_conv_stats`` (section 27) terms of the block's ``bn_act`` sums — no ATen normalisation is left.

``UNetPyramid`` holds what one batch needs, built once (``build_unet_pyramid``): five levels at tensor strides 1 .. 16 — the
coordinate sets ``build_pyramid`` gives —, per level the kernel-3 and the kernel-1 map, at level 0 the stem's map, between
neighbouring levels the octant map.

Inference (``tuning.override(eval_epilogue=True)``, a fused network in eval mode with autograd disabled): every convolution + norm
is ONE library call (``Res16UNetBase._forward_infer``) — ``sparse_conv_bn_act`` (section 19) for the kernel-3 / kernel-1
convolutions, ``octant_conv_bn_act`` (section 23) for the eight resolution changes.  A decoder level's ``[up | skip]`` input is one
buffer that the transposed convolution and the launch that produces the skip map write their column blocks of; a block that reads
more than 256 columns runs ``conv1`` and the ``downsample`` convolution as a chain of two launches over the two column blocks.

Offset and octant numbering and the sorted order of the coarse levels are this project's choice (minkowski_conv.py): parity unpinned
against MinkowskiEngine's own checkpoints.  The switch ``grouped_passes`` of ``tuning`` leaves these networks as they are;
``rows_single_product`` reaches the kernel-3 / kernel-1 convolutions as everywhere, in training and on the inference graph, and
by itself never the octant products (sections 21 and 23 have no single-product instances).  ``infer_maps16`` (16-bit maps between
the launches of ``HRNetBackbone``'s inference graph) is ignored here.  The inference graph has two switches of its own, which act
where ``eval_epilogue`` acts on these networks AND ``maps16_dtype()`` is not None (math mode "bf16" / "fp16" with
``rows_single_product``) and change nothing anywhere else: ``octant_single_product`` runs the eight resolution changes as ONE 16-bit
product (section 25) on fp32 maps; ``unet_maps16`` implies that and stores every map between the launches as a bf16 / fp16 tensor
(sections 24 and 25) — the ``[up | skip]`` buffers included, written in place by their two producers as before.  The stem's input, a
chain's running sum (an fp32 scratch map: the sum is rounded once, like every other stored map) and the last block's output, which
``final`` reads, stay fp32.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as CF
from . import minkowski_conv as _mc
from . import minkowski_hrnet as _mh
from . import tuning
from .minkowski_conv import (KernelMap, OctantMap, SparseConv3d, SparseConvDown2, SparseConvUp2, build_kernel_map, build_octant_map,
                             cat_conv3d)
from .minkowski_hrnet import (HRBasicBlock, VoxelPyramid, _combine, _conv_bn, _conv_bn_act, _keep, _pitched, _pitched16, _rows_any,
                              maps16_dtype, sparse_conv_bn_act)

_NO_CPU = "csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path"
N_LEVELS = 5


class UNetPyramid:
    """Coordinates and maps of one batch for a Res16UNet: ``coords[l]`` (n_l, 4) at tensor stride 2^l for l = 0 .. 4; ``s1[l]`` the
    kernel-3 stride-1 map of level l; ``one[l]`` its kernel-1 map (the blocks' ``downsample``); ``stem`` the kernel-``stem_kernel``
    map of level 0; ``oct[l]`` the octant map from level l onto level l + 1 (both directions)."""

    def __init__(self, coords: List[torch.Tensor], s1: List[KernelMap], one: List[KernelMap], stem: KernelMap, oct: List[OctantMap],
                 stem_kernel: int):
        self.coords, self.s1, self.one, self.stem, self.oct, self.stem_kernel = coords, s1, one, stem, oct, stem_kernel

    def to(self, device) -> "UNetPyramid":
        return UNetPyramid([c.to(device) for c in self.coords], [m.to(device) for m in self.s1], [m.to(device) for m in self.one],
                           self.stem.to(device), [m.to(device) for m in self.oct], self.stem_kernel)


def build_unet_pyramid(coords: torch.Tensor, stem_kernel: int = 5, backend: Optional[str] = None) -> UNetPyramid:
    """The pyramid of ``coords`` (n, 4) = [b, x, y, z] at tensor stride 1 (device or CPU tensor; the maps live where it does).
    ``backend`` as in ``build_kernel_map``: ``"torch"``, ``"hip"`` (device tensors only) or None for the tuning switch
    ``native_kernel_maps``; both give the same pyramid, kernel maps and octant maps alike."""
    backend = _mc.resolve_backend(backend, coords)
    if backend == "hip":
        return _build_unet_pyramid_hip(coords, stem_kernel)
    levels, s1, one, octs = [coords.long()], [], [], []
    for l in range(N_LEVELS):
        ts = 1 << l
        s1.append(build_kernel_map(levels[l], kernel_size=3, stride=1, tensor_stride=ts, backend=backend))
        one.append(build_kernel_map(levels[l], kernel_size=1, stride=1, tensor_stride=ts, backend=backend))
        if l + 1 < N_LEVELS:
            octs.append(build_octant_map(levels[l], tensor_stride=ts, backend=backend))
            levels.append(octs[-1].out_coords)
    stem = s1[0] if stem_kernel == 3 else build_kernel_map(levels[0], kernel_size=stem_kernel, stride=1, tensor_stride=1,
                                                           backend=backend)
    return UNetPyramid(levels, s1, one, stem, octs, stem_kernel)


def _build_unet_pyramid_hip(coords: torch.Tensor, stem_kernel: int) -> UNetPyramid:
    """The same pyramid on include/csn_hip.h sections 17 and 22, in the manner of ``minkowski_hrnet._build_pyramid_hip``.  Level l's
    keys and their sort are formed once and serve ``s1[l]``, ``one[l]``, the stem and ``oct[l]``; a coarser level leaves
    ``torch.unique`` sorted, so it is never sorted again.  Level 0 takes one key launch; a coarser level one launch for the floored
    keys and one key launch on its unpacked coordinates (the level's range and tensor-stride check, as in the HRNet's pyramid); one
    lookup launch per table — five kernel-3, five kernel-1, the stem's —; per octant map one partition call and one order call.  The
    kernel-3 lookup of a level has checked its sorted keys' neighbours, so the partition is not handed them again.  One status word
    for the whole pyramid, read once at the end: 5 + 4 + 11 + 4 + 4 = 28 library calls (27 with a kernel-3 stem) and one host read."""
    if stem_kernel < 1 or stem_kernel % 2 == 0:
        raise ValueError(f"kernel_size {stem_kernel} is not supported: odd sizes only")
    if stem_kernel not in (1, 3, 5):
        raise ValueError(f"kernel_size {stem_kernel} is not supported: the kernels take 1, 3 and 5")
    status = _mc._new_status(coords.device)
    sets, s1, one, octs = [_mc._key_set(coords, 1, "coords", status)], [], [], []
    for l in range(N_LEVELS):
        ts, here = 1 << l, sets[l]
        s1.append(KernelMap(here.coords, here.coords, 3, 1, ts, ts, False, _mc._lookup(here, here, 3, ts, status), None))
        one.append(KernelMap(here.coords, here.coords, 1, 1, ts, ts, False, _mc._lookup(here, here, 1, ts, status), None))
        if l + 1 < N_LEVELS:
            up = _mc._coarse_set(here, 2 * ts)
            up.keys = _mc._coord_keys(up.coords, 2 * ts, status)
            sets.append(up)
            octs.append(_mc._octant_map(here, up, ts, status, False))
    if stem_kernel == 3:
        stem = s1[0]
    else:
        stem = KernelMap(sets[0].coords, sets[0].coords, stem_kernel, 1, 1, 1, False,
                         _mc._lookup(sets[0], sets[0], stem_kernel, 1, status), None)
    _mc._raise_for_status(_mc._read_status(status), [(coords, 1, "coords")])
    return UNetPyramid([s.coords for s in sets], s1, one, stem, octs, stem_kernel)


# ------------------------------------------------------------------------------------------------------
# inference: an octant convolution + BatchNorm + residual + ReLU as one launch (sections 23 and 25)
# ------------------------------------------------------------------------------------------------------
def octant_conv_bn_act(x: torch.Tensor, weight: torch.Tensor, omap: OctantMap, norm: nn.BatchNorm1d, up: bool,
                       residual: Optional[torch.Tensor] = None, relu: bool = True, out: Optional[torch.Tensor] = None, *,
                       out_dtype: Optional[torch.dtype] = None, single_product: bool = False) -> torch.Tensor:
    """``y = act(conv(x) s + t + residual)`` in one launch, the counterpart of ``sparse_conv_bn_act`` for the kernel-2 stride-2
    convolution (``up`` False: ``x (n_fine, c_in)`` -> ``(n_coarse, c_out)``, ``csn_octant_down_bn_act_fwd_f32``) and its transposed
    form (``up`` True: ``x (n_coarse, c_in)`` -> ``(n_fine, c_out)``, ``csn_octant_up_bn_act_fwd_f32``), both without a bias:
    ``weight (8, c_in, c_out)``, ``s = gamma / sqrt(running_var + eps)``, ``t = beta - running_mean s`` from ``norm``'s running
    statistics, ``act`` the ReLU or the identity.  Inference only: no autograd node, the result has no ``grad_fn``.

    ``x``, ``residual`` and ``out`` may be row-pitched views of a wider buffer (``stride(1) == 1``, ``stride(0) % 4 == 0``, a
    16-byte aligned data pointer); ``x`` and ``residual`` are made contiguous otherwise, ``out`` raises ``ValueError``.  With
    ``out`` the result is written there and ``out`` is returned; ``residual`` may be ``out`` itself and must not overlap it in any
    other way.  The products run in fp32 (math mode 0) or as bf16x3 (every other mode), whatever ``rows_single_product`` says.

    Single product and 16-bit maps (``csn_octant_down_bn_act_fwd_m16`` / ``csn_octant_up_bn_act_fwd_m16``, section 25).  In math
    mode "bf16" / "fp16" with ``tuning.rows_single_product``, ``single_product=True`` runs ONE 16-bit product per operand pair, and
    ``x``, ``residual`` and ``out`` may each be fp32 or that mode's 16-bit dtype (16-bit views need ``stride(0) % 8 == 0``);
    ``out_dtype`` names the type of a result allocated here.  Any of these takes that route; without the mode and the switch, or
    with a tensor of the other 16-bit type, it raises ``ValueError``.  A launch on 16-bit maps is bit-identical to the
    ``single_product=True`` launch on the same values in fp32 maps, its result rounded once (nearest even) where the output is
    16-bit.  Calls on fp32 tensors without ``out_dtype`` and ``single_product`` are section 23 as ever."""
    named = out_dtype if out_dtype is not None or not single_product else (torch.float32 if out is None else out.dtype)
    dt16 = _mh._maps16_route(x, residual, out, named)
    if not (x.is_cuda and weight.is_cuda) or (residual is not None and not residual.is_cuda) or (out is not None and not out.is_cuda):
        raise _lib.CsnError(_NO_CPU)
    if not isinstance(omap, OctantMap):
        raise ValueError(f"a kernel-2 stride-2 convolution takes an OctantMap, not {type(omap).__name__}")
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1] or weight.shape[0] != 8:
        raise ValueError("x must be (n_in, c_in) and weight (8, c_in, c_out)")
    n_fine, n_coarse = omap.n_fine, omap.n_coarse
    n_in, n_out = (n_coarse, n_fine) if up else (n_fine, n_coarse)
    if x.shape[0] != n_in:
        raise ValueError(f"x has {x.shape[0]} rows, the map's input set {n_in}")
    _, c_in, c_out = weight.shape
    for name, c in (("c_in", c_in), ("c_out", c_out)):
        if c % 32 or not 32 <= c <= 256:
            raise ValueError(f"{name} {c} is not supported: a multiple of 32 in [32, 256]")
    if not isinstance(norm, nn.BatchNorm1d) or norm.num_features != c_out or norm.running_mean is None or norm.weight is None:
        raise ValueError(f"norm must be an affine nn.BatchNorm1d({c_out}) that tracks running statistics")
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and tuple(t.shape) != (n_out, c_out):
            raise ValueError(f"{name} must be ({n_out}, {c_out})")
    CF._need_cuda(omap.parent, norm.weight, norm.bias, norm.running_mean, norm.running_var)
    same = residual is not None and out is not None and residual.data_ptr() == out.data_ptr() and residual.stride() == out.stride()
    w = weight.detach().float().contiguous()
    x = _rows_any(x)
    if out is None:
        y = torch.empty((n_out, c_out), device=x.device, dtype=out_dtype or torch.float32)
    else:
        y = out.detach()
        if not (_pitched(y) or (dt16 is not None and _pitched16(y))):
            raise ValueError("out must be fp32 rows with stride(1) == 1, stride(0) % 4 == 0 and a 16-byte aligned data pointer"
                             + ("" if dt16 is None else f", or {dt16} rows with stride(0) % 8 == 0"))
    r = None if residual is None else (y if same else _rows_any(residual))
    vec = [CF._ptr(v.detach().float().contiguous()) for v in (norm.weight, norm.bias, norm.running_mean, norm.running_var)]
    if dt16 is not None:
        is16 = lambda t: int(t is not None and t.dtype == dt16)
        tail16 = (float(norm.eps), CF._ptr(r), is16(r), 0 if r is None else r.stride(0), int(bool(relu)), CF._ptr(y), is16(y), y.stride(0),
                  CF._stream())
        L = _lib.lib()
        with CF.rows16(True):
            if up:
                _lib.check(L.csn_octant_up_bn_act_fwd_m16(CF._ptr(x), is16(x), x.stride(0), n_coarse, CF._ptr(omap.parent),
                                                          CF._ptr(omap.order), CF._ptr(omap.seg), n_fine, c_in, c_out, CF._ptr(w), *vec,
                                                          *tail16), "csn_octant_up_bn_act_fwd_m16")
            else:
                _lib.check(L.csn_octant_down_bn_act_fwd_m16(CF._ptr(x), is16(x), x.stride(0), n_fine, CF._ptr(omap.children), n_coarse,
                                                            c_in, c_out, CF._ptr(w), *vec, *tail16), "csn_octant_down_bn_act_fwd_m16")
        return y if out is None else out
    tail = (float(norm.eps), CF._ptr(r), 0 if r is None else r.stride(0), int(bool(relu)), CF._ptr(y), y.stride(0), CF._stream())
    L = _lib.lib()
    if up:
        _lib.check(L.csn_octant_up_bn_act_fwd_f32(CF._ptr(x), x.stride(0), n_coarse, CF._ptr(omap.parent), CF._ptr(omap.order),
                                                  CF._ptr(omap.seg), n_fine, c_in, c_out, CF._ptr(w), *vec, *tail),
                   "csn_octant_up_bn_act_fwd_f32")
    else:
        _lib.check(L.csn_octant_down_bn_act_fwd_f32(CF._ptr(x), x.stride(0), n_fine, CF._ptr(omap.children), n_coarse, c_in, c_out,
                                                    CF._ptr(w), *vec, *tail), "csn_octant_down_bn_act_fwd_f32")
    return y if out is None else out


def _octant_bn_act(conv: SparseConvDown2, norm: nn.BatchNorm1d, x, omap: OctantMap, residual=None, relu=True, out=None, out_dtype=None,
                   single_product=False) -> torch.Tensor:
    if conv.bias is not None:
        raise ValueError("the inference launch of an octant convolution takes no bias (the Res16UNets have none)")
    return octant_conv_bn_act(x, conv.kernel, omap, norm, conv.up, residual, relu, out, out_dtype=out_dtype, single_product=single_product)


# ------------------------------------------------------------------------------------------------------
# training: the octant products and the convolution over a concatenation with the BatchNorm statistics epilogue (sections 26, 27)
# ------------------------------------------------------------------------------------------------------
class _OctantConvStats(torch.autograd.Function):
    """(z, mean, invstd) = ``csn_octant_{down,up}_stats_fwd_f32``; updates the running statistics in place.  mean / invstd are
    constants of the graph; the backward is ``csn_octant_{down,up}_bwd_f32`` with dbias = NULL."""

    @staticmethod
    def forward(ctx, x, w, omap, up, running_mean, running_var, eps, momentum):
        CF._need_cuda(x, w, omap.parent, running_mean, running_var)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        x = x.contiguous()
        w_c = w.detach().contiguous()
        _, c_in, c_out = w_c.shape
        n_fine, n_coarse = omap.n_fine, omap.n_coarse
        ws_n = int(L.csn_octant_stats_workspace_bytes(n_fine, n_coarse, c_out, int(up)))
        z, mean, invstd, ws = _mh._stats_outputs(n_fine if up else n_coarse, c_out, ws_n, x.device)
        tail = (CF._ptr(w_c), CF._ptr(z), c_out, CF._ptr(mean), CF._ptr(invstd), CF._ptr(running_mean), CF._ptr(running_var), float(eps),
                float(momentum), CF._ptr(ws), ws_n, CF._stream())
        if up:
            _lib.check(L.csn_octant_up_stats_fwd_f32(CF._ptr(x), c_in, n_coarse, CF._ptr(omap.parent), CF._ptr(omap.order),
                                                     CF._ptr(omap.seg), n_fine, c_in, c_out, *tail), "csn_octant_up_stats_fwd_f32")
        else:
            _lib.check(L.csn_octant_down_stats_fwd_f32(CF._ptr(x), c_in, n_fine, CF._ptr(omap.children), n_coarse, c_in, c_out, *tail),
                       "csn_octant_down_stats_fwd_f32")
        ctx.save_for_backward(x, w_c)
        ctx.omap, ctx.up = omap, up
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dmean, _dinvstd):
        with CF.math_mode(CF.backward_mode(ctx.mode)):
            x, w = ctx.saved_tensors
            dx, dw, _ = _mc._octant_conv_backward(dz, x, w, ctx.omap, ctx.up, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
            return (dx, dw) + (None,) * 6


def octant_conv_stats(x: torch.Tensor, weight: torch.Tensor, omap: OctantMap, up: bool, running_mean: Optional[torch.Tensor],
                      running_var: Optional[torch.Tensor], eps: float, momentum: float):
    """``z``, ``mean``, ``invstd`` of the kernel-2 stride-2 convolution (``up`` False: ``x (n_fine, c_in)`` -> ``z (n_coarse,
    c_out)``) or its transposed form (``up`` True: ``x (n_coarse, c_in)`` -> ``z (n_fine, c_out)``) without a bias, and of ``z``'s
    BatchNorm batch, formed by the product's own epilogue (include/csn_hip.h section 26); the running statistics (either may be
    None) are updated in place.  ``z`` holds the bits of ``octant_conv_down`` / ``octant_conv_up``.  ``weight (8, c_in, c_out)``,
    widths multiples of 32 in [32, 256].  The statistics are constants of the graph: feed ``(z, mean, invstd, gamma, beta)`` to
    ``bn_act``, whose backward is the complete BatchNorm gradient.  A one-row ``z`` raises ``ValueError`` (no variance)."""
    if not (x.is_cuda and weight.is_cuda):
        raise _lib.CsnError(_NO_CPU)
    if not isinstance(omap, OctantMap):
        raise ValueError(f"a kernel-2 stride-2 convolution takes an OctantMap, not {type(omap).__name__}")
    if x.dim() != 2 or weight.dim() != 3 or x.shape[1] != weight.shape[1] or weight.shape[0] != 8:
        raise ValueError("x must be (n_in, c_in) and weight (8, c_in, c_out)")
    n_in, n_out = (omap.n_coarse, omap.n_fine) if up else (omap.n_fine, omap.n_coarse)
    if x.shape[0] != n_in:
        raise ValueError(f"x has {x.shape[0]} rows, the map's input set {n_in}")
    for name, c in (("c_in", weight.shape[1]), ("c_out", weight.shape[2])):
        if c % 32 or not 32 <= c <= 256:
            raise ValueError(f"{name} {c} is not supported: a multiple of 32 in [32, 256]")
    if n_out < 2:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    return _OctantConvStats.apply(x.float(), weight, omap, bool(up), running_mean, running_var, eps, momentum)


class _CatConvStats(torch.autograd.Function):
    """(z, mean, invstd) = ``csn_sparse_conv_cat_stats_fwd_f32`` on the parts as they lie (row-pitched views are handed over with
    their pitch); updates the running statistics in place.  The backward is ``csn_sparse_conv_bwd_f32`` per part on a contiguous
    copy of that part's slice of the kernel; dw is written slice by slice into one (KV, sum c_in, c_out) tensor.
    Arguments after the fixed ones: the parts."""

    @staticmethod
    def forward(ctx, w, kmap, running_mean, running_var, eps, momentum, *parts):
        CF._need_cuda(w, kmap.fwd, running_mean, running_var, *parts)
        L = _lib.lib()
        ctx.mode = CF.current_mode()
        ctx.rows16 = tuning.current().rows_single_product
        xs = [_mh._rows(p) for p in parts]
        w_c = w.detach().contiguous()
        KV, _, c_out = w_c.shape
        n_in, n_out = kmap.n_in, kmap.n_out
        ws_n = int(L.csn_sparse_conv_cat_stats_workspace_bytes(n_out, c_out))
        z, mean, invstd, ws = _mh._stats_outputs(n_out, c_out, ws_n, w_c.device)
        cp = _lib.CatParts()
        for m, x in enumerate(xs):
            cp.x[m], cp.ld_x[m], cp.c_in[m] = x.data_ptr(), x.stride(0), x.shape[1]
        with CF.rows16(ctx.rows16):
            _lib.check(L.csn_sparse_conv_cat_stats_fwd_f32(ctypes.byref(cp), len(xs), n_in, CF._ptr(kmap.fwd), n_out, KV, c_out,
                                                           CF._ptr(w_c), CF._ptr(z), c_out, CF._ptr(mean), CF._ptr(invstd),
                                                           CF._ptr(running_mean), CF._ptr(running_var), float(eps), float(momentum),
                                                           CF._ptr(ws), ws_n, CF._stream()), "csn_sparse_conv_cat_stats_fwd_f32")
        ctx.save_for_backward(w_c, *xs)
        ctx.kmap = kmap
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dmean, _dinvstd):
        with CF.math_mode(CF.backward_mode(ctx.mode)), CF.rows16(ctx.rows16):
            w, *xs = ctx.saved_tensors
            need_w = ctx.needs_input_grad[0]
            need_x = [ctx.needs_input_grad[6 + m] for m in range(len(xs))]
            if not (need_w or any(need_x)):
                return (None,) * (6 + len(xs))
            dz = dz.contiguous()
            dw = torch.empty_like(w) if need_w else None
            dxs, c0 = [], 0
            for x, nx in zip(xs, need_x):
                c_in = int(x.shape[1])
                w_m = w[:, c0:c0 + c_in].contiguous() if nx else None
                dx, dw_m, _ = _mc._sparse_conv_backward(dz, x, x.stride(0), w_m, ctx.kmap, nx, need_w)
                if need_w:
                    dw[:, c0:c0 + c_in] = dw_m
                dxs.append(dx)
                c0 += c_in
            return (dw, None, None, None, None, None, *dxs)


def cat_conv_stats(parts: Sequence[torch.Tensor], weight: torch.Tensor, kmap: KernelMap, running_mean: Optional[torch.Tensor],
                   running_var: Optional[torch.Tensor], eps: float, momentum: float):
    """``z (n_out, c_out)``, ``mean``, ``invstd`` of the convolution of ``torch.cat(parts, dim=1)`` and of its BatchNorm batch
    (include/csn_hip.h section 27): ``parts`` 1 to 4 maps ``(n_in, c_p)``, every ``c_p`` a multiple of 32 in [32, 256], and
    ``weight (KV, sum c_p, c_out)`` ONE kernel (kernel size 1 or 3), read in place through each part's row offset.  The
    concatenation is never formed: a chain of one launch per part, the last of which forms the statistics of the completed sum.
    Parts that are column blocks of one wider buffer are read through their pitch.  The running statistics (either may be None)
    are updated in place.  With one part it is ``conv_stats``, bit for bit.  A one-row output raises ``ValueError``."""
    parts = list(parts)
    if not 1 <= len(parts) <= 4:
        raise ValueError(f"cat_conv_stats takes 1 to 4 parts, not {len(parts)}")
    if not (weight.is_cuda and all(p.is_cuda for p in parts)):
        raise _lib.CsnError(_NO_CPU)
    if weight.dim() != 3 or any(p.dim() != 2 for p in parts) or sum(int(p.shape[1]) for p in parts) != weight.shape[1]:
        raise ValueError("the parts must be (n_in, c_p) maps whose widths add up to the weight's c_in")
    if weight.shape[0] != kmap.KV or kmap.KV not in (1, 27) or any(p.shape[0] != kmap.n_in for p in parts):
        raise ValueError("weight must be (KV, c_in, c_out) for the map's KV (kernel size 1 or 3) and every part must have its n_in rows")
    c_out = weight.shape[2]
    if c_out % 32 or not 32 <= c_out <= 256 or any(p.shape[1] % 32 or not 32 <= p.shape[1] <= 256 for p in parts):
        raise ValueError("widths: c_out and every part a multiple of 32 in [32, 256]")
    if kmap.n_out < 2:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    return _CatConvStats.apply(weight, kmap, running_mean, running_var, eps, momentum, *[p.float() for p in parts])


class CatConv3d(nn.Module):
    """A stride-1 convolution whose input is a concatenation wider than 256 columns: it holds MinkowskiEngine's ``kernel (KV,
    c_in, c_out)`` and runs ``cat_conv3d`` on the parts."""

    stride, transposed = 1, False

    def __init__(self, c_in: int, c_out: int, kernel_size: int = 3):
        super().__init__()
        if kernel_size not in (1, 3, 5):
            raise ValueError(f"kernel_size {kernel_size} is not supported: 1, 3 or 5")
        if c_out % 32 or not 32 <= c_out <= 256 or c_in < 1:
            raise ValueError("widths: c_out a multiple of 32 in [32, 256]")
        self.c_in, self.c_out, self.kernel_size = c_in, c_out, kernel_size
        KV = kernel_size ** 3
        self.kernel = nn.Parameter(torch.empty(KV, c_in, c_out))
        nn.init.normal_(self.kernel, std=(KV * c_in) ** -0.5)

    def forward(self, parts: Sequence[torch.Tensor], kmap: KernelMap) -> torch.Tensor:
        if kmap.kernel_size != self.kernel_size or kmap.stride != 1 or kmap.transposed:
            raise ValueError(f"the map (kernel {kmap.kernel_size}, stride {kmap.stride}, transposed {kmap.transposed}) does not fit "
                             f"this layer (kernel {self.kernel_size}, stride 1, transposed False)")
        return cat_conv3d(parts, self.kernel, kmap)

    def extra_repr(self) -> str:
        return f"{self.c_in}, {self.c_out}, kernel_size={self.kernel_size}, stride=1, bias=False"


def _cat_conv_bn(conv: CatConv3d, norm: nn.BatchNorm1d, parts: Sequence[torch.Tensor], kmap: KernelMap):
    """``_conv_bn`` for a convolution over a concatenation, training mode on the fused nodes: the term (z, mean, invstd, gamma, beta)
    of ``bn_act``; the norm's running statistics and ``num_batches_tracked`` advance as ATen's do."""
    if kmap.kernel_size != conv.kernel_size or kmap.stride != 1 or kmap.transposed:
        raise ValueError(f"the map (kernel {kmap.kernel_size}, stride {kmap.stride}, transposed {kmap.transposed}) does not fit "
                         f"this layer (kernel {conv.kernel_size}, stride 1, transposed False)")
    if kmap.n_out == 1:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    norm.num_batches_tracked += 1
    z, mean, invstd = cat_conv_stats(parts, conv.kernel, kmap, norm.running_mean, norm.running_var, norm.eps, norm.momentum)
    return (z, mean, invstd, norm.weight, norm.bias)


def _octant_bn_relu(conv: SparseConvDown2, norm: nn.BatchNorm1d, x: torch.Tensor, omap: OctantMap, tail: bool) -> torch.Tensor:
    """relu(norm(conv(x))) of a resolution change.  ``tail`` (``tuning.unet_fused_tail``, a fused network in training mode):
    ``octant_conv_stats`` + ``bn_act`` (section 26 + 15b) instead of the octant node + ATen's BatchNorm + ``F.relu``."""
    if not tail:
        return F.relu(norm(conv(x, omap)))
    if conv.bias is not None:
        raise ValueError("the statistics launch of an octant convolution takes no bias (the Res16UNets have none)")
    n_out = omap.n_fine if conv.up else omap.n_coarse
    if n_out == 1:
        raise ValueError("Expected more than 1 value per channel when training (a one-row batch has no variance)")
    norm.num_batches_tracked += 1
    z, mean, invstd = octant_conv_stats(x, conv.kernel, omap, conv.up, norm.running_mean, norm.running_var, norm.eps, norm.momentum)
    return _mh.bn_act([(z, mean, invstd, norm.weight, norm.bias)], None, True, True, norm.eps)


class UNetBasicBlock(nn.Module):
    """``BasicBlock`` of resnet_block.py:22-57 with the ``downsample`` of resnet.py:96-107 (``downsample.0`` the kernel-1
    convolution, ``downsample.1`` its BatchNorm): conv1 - norm1 - relu - conv2 - norm2, plus norm(downsample(x)), relu.  ``forward``
    takes the input as a list of parts ``[up, skip]`` (or ``[x]``) with the level's kernel-3 and kernel-1 maps; ``trace`` (a dict)
    receives the two ReLU outputs under ``prefix + "norm1"`` / ``prefix + "norm2"``, as in ``HRBasicBlock``."""

    expansion = 1

    def __init__(self, inplanes: int, planes: int, bn_momentum: float = 0.02, fused: bool = True):
        super().__init__()
        conv = SparseConv3d if inplanes <= 256 else CatConv3d
        self.conv1 = conv(inplanes, planes, kernel_size=3)
        self.norm1 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.conv2 = SparseConv3d(planes, planes, kernel_size=3)
        self.norm2 = nn.BatchNorm1d(planes, momentum=bn_momentum)
        self.downsample = nn.Sequential(conv(inplanes, planes, kernel_size=1), nn.BatchNorm1d(planes, momentum=bn_momentum))
        self.inplanes, self.fused = inplanes, fused

    def forward(self, parts: Sequence[torch.Tensor], s1: KernelMap, one: KernelMap, trace: Optional[dict] = None,
                prefix: str = "") -> torch.Tensor:
        f, tr = self.fused, self.training
        if sum(int(p.shape[1]) for p in parts) != self.inplanes:
            raise ValueError(f"the parts are {[int(p.shape[1]) for p in parts]} wide; this block takes {self.inplanes} columns")
        if not all(p.is_cuda for p in parts):
            raise _lib.CsnError(_NO_CPU)
        ds_conv, ds_norm = self.downsample[0], self.downsample[1]
        if self.inplanes <= 256:
            x = parts[0] if len(parts) == 1 else torch.cat(list(parts), dim=1)
            out = _combine([_conv_bn(self.conv1, self.norm1, x, s1, f)], f, tr, self.norm1.eps)
            res = _conv_bn(ds_conv, ds_norm, x, one, f)
        elif f and tr and tuning.current().unet_fused_tail:
            # the split path on the fused nodes: each of the two convolutions is a chain over the parts whose last launch forms the
            # BatchNorm statistics (section 27); the terms join the block's bn_act sums like any other
            out = _combine([_cat_conv_bn(self.conv1, self.norm1, parts, s1)], f, tr, self.norm1.eps)
            res = _cat_conv_bn(ds_conv, ds_norm, parts, one)
        else:
            # the split path: the two convolutions that read the concatenation are sums over its parts; their norms are ATen's
            out = F.relu(self.norm1(self.conv1(parts, s1)))
            res = ("r", ds_norm(ds_conv(parts, one)))
        _keep(trace, prefix + "norm1", out)
        return _keep(trace, prefix + "norm2", _combine([_conv_bn(self.conv2, self.norm2, out, s1, f), res], f, tr, self.norm2.eps))

    def _column_kernels(self, conv, widths: Sequence[int]) -> List[torch.Tensor]:
        """``conv.kernel`` cut along c_in into contiguous (KV, w, c_out) pieces, made once per state of the parameter."""
        key = (conv.kernel.data_ptr(), conv.kernel._version, tuple(widths))
        cache = self.__dict__.setdefault("_cut", {})
        if cache.get(id(conv), (None,))[0] != key:
            cache[id(conv)] = (key, [k.contiguous() for k in conv.kernel.detach().float().split(list(widths), dim=1)])
        return cache[id(conv)][1]

    def _infer_conv(self, conv, norm: nn.BatchNorm1d, x: torch.Tensor, kmap: KernelMap, widths: Sequence[int], relu: bool,
                    dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """One convolution + norm that reads the block's input: one launch up to 256 columns; beyond, a chain over the input's
        column blocks ``widths`` (each a multiple of 32, at most 256): the first launch writes ``z0 s + t`` without a ReLU, each
        further one adds its ``z_i s`` to that map in place (zero shift) and the last applies the activation.  ``dtype`` (16-bit
        maps, ``tuning.unet_maps16``): the type of the result; a chain then keeps its running sum in an fp32 scratch map and its
        last launch reads that and writes the 16-bit map, so that the sum is rounded once."""
        if isinstance(conv, SparseConv3d):
            return _conv_bn_act(conv, norm, x, kmap, relu=relu, out_dtype=dtype)
        if kmap.kernel_size != conv.kernel_size or kmap.stride != 1 or kmap.transposed:
            raise ValueError("the map does not fit this layer")
        if sum(widths) != self.inplanes or any(w % 32 or not 32 <= w <= 256 for w in widths):
            raise ValueError(f"column blocks {list(widths)} do not cut {self.inplanes} columns into multiples of 32 up to 256")
        y, c0 = None, 0
        for i, (w, k) in enumerate(zip(widths, self._column_kernels(conv, widths))):
            last = i == len(widths) - 1
            if dtype is None:
                y = sparse_conv_bn_act(x[:, c0:c0 + w], k, kmap, norm, residual=y, relu=relu and last, out=y, shift=i == 0)
            elif last:
                y = sparse_conv_bn_act(x[:, c0:c0 + w], k, kmap, norm, residual=y, relu=relu, shift=i == 0, out_dtype=dtype)
            else:
                y = sparse_conv_bn_act(x[:, c0:c0 + w], k, kmap, norm, residual=y, relu=False, out=y, shift=i == 0,
                                       out_dtype=torch.float32 if y is None else None)
            c0 += w
        return y

    def infer(self, x: torch.Tensor, s1: KernelMap, one: KernelMap, trace: Optional[dict] = None, prefix: str = "",
              out: Optional[torch.Tensor] = None, widths: Optional[Sequence[int]] = None, dtype: Optional[torch.dtype] = None,
              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """The block on the inference launches, ``x (n, inplanes)`` a map or the level's ``[up | skip]`` buffer: ``conv1`` + ``norm1``
        + ReLU, the ``downsample`` convolution + its norm without a ReLU, ``conv2`` + ``norm2`` with that result as its residual,
        then the ReLU (written to ``out`` when given, else in place over the residual).  ``widths``: the column blocks of a wider
        input (default: 256 and the rest); the two convolutions that read it are then chains, ``(z0 s + t) + z1 s`` — a summation
        order of its own, neither ``cat_conv3d``'s ``z0 + z1`` nor the one launch's.  ``dtype`` (16-bit maps,
        ``tuning.unet_maps16``): the type of the two inner maps; ``out_dtype``: that of a result allocated here (a result of another
        type than the residual map is a map of its own)."""
        if not x.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if x.dim() != 2 or x.shape[1] != self.inplanes:
            raise ValueError(f"x is {tuple(x.shape)}; this block takes {self.inplanes} columns")
        if widths is None:
            widths = [self.inplanes] if self.inplanes <= 256 else [256, self.inplanes - 256]
        h = _keep(trace, prefix + "norm1", self._infer_conv(self.conv1, self.norm1, x, s1, widths, True, dtype))
        res = self._infer_conv(self.downsample[0], self.downsample[1], x, one, widths, False, dtype)
        if out is None and (out_dtype is None or out_dtype == res.dtype):
            out = res
        return _keep(trace, prefix + "norm2", _conv_bn_act(self.conv2, self.norm2, h, s1, residual=res, out=out,
                                                           out_dtype=None if out is not None else out_dtype))


class Res16UNetBase(nn.Module):
    """``Res16UNetBase`` (res16unet.py:11-229) with the reference's attribute names: ``conv0p1s1`` / ``bn0``, ``conv{1..4}p{1,2,4,
    8}s2`` / ``bn{1..4}``, ``block1`` .. ``block8`` (``nn.Sequential`` of blocks: ``blockN.i.conv1.kernel``, ``.norm1.*``,
    ``.downsample.0.kernel``, ``.downsample.1.*``), ``convtr{4..7}p{16,8,4,2}s2`` / ``bntr{4..7}``, ``final`` (the kernel-1 output
    convolution as an ``nn.Linear`` with bias).

    ``forward((coords, feats))``: ``coords (N, 4)`` rows [b, x, y, z] (or a ``UNetPyramid`` built for them, or a ``VoxelPyramid``,
    whose level-0 coordinates are taken), ``feats (N, in_channels)``; returns the (N, out_channels) logits, in training and eval.
    ``trace``: a dict that receives every ReLU's output, keyed ``bn0`` .. ``bn4``, ``bntr4`` .. ``bntr7`` and
    ``blockN.i.norm1`` / ``.norm2``."""

    PLANES = (32, 64, 128, 256, 256, 256, 256, 256)
    LAYERS = (2, 2, 2, 2, 2, 2, 2, 2)
    INIT_DIM = 32
    BLOCK = "BasicBlock"
    NORM_TYPE = "BATCH_NORM"

    def __init__(self, in_channels: int, out_channels: int, bn_momentum: float = 0.02, conv1_kernel_size: int = 5, fused: bool = True):
        super().__init__()
        name = type(self).__name__
        if self.BLOCK != "BasicBlock":
            raise NotImplementedError(f"{name} is built from Bottleneck blocks, whose inner widths (planes // 4 = 8, 16, 24, ...) are no "
                                      "multiples of 32; the kernels take widths that are")
        if self.NORM_TYPE != "BATCH_NORM":
            raise NotImplementedError(f"{name}: norm type {self.NORM_TYPE} is not supported: BatchNorm only")
        if max(self.PLANES) > 256:
            raise NotImplementedError(f"{name} needs {max(self.PLANES)}-wide convolutions; the kernels (include/csn_hip.h sections 14 "
                                      "and 21) take widths up to 256")
        P, self.fused, self.conv1_kernel_size = self.PLANES, fused, conv1_kernel_size
        mom = bn_momentum
        bn = lambda c: nn.BatchNorm1d(c, momentum=mom)
        self.inplanes = self.INIT_DIM
        self.conv0p1s1 = SparseConv3d(in_channels, self.inplanes, kernel_size=conv1_kernel_size)
        self.bn0 = bn(self.inplanes)
        for n, ts in ((1, 1), (2, 2), (3, 4), (4, 8)):
            setattr(self, f"conv{n}p{ts}s2", SparseConvDown2(self.inplanes, self.inplanes))
            setattr(self, f"bn{n}", bn(self.inplanes))
            setattr(self, f"block{n}", self._make_layer(P[n - 1], self.LAYERS[n - 1], mom))
        skips = (P[2], P[1], P[0], self.INIT_DIM)
        for n, ts in ((4, 16), (5, 8), (6, 4), (7, 2)):
            setattr(self, f"convtr{n}p{ts}s2", SparseConvUp2(self.inplanes, P[n]))
            setattr(self, f"bntr{n}", bn(P[n]))
            self.inplanes = P[n] + skips[n - 4]
            setattr(self, f"block{n + 1}", self._make_layer(P[n], self.LAYERS[n], mom))
        self.final = nn.Linear(P[7], out_channels, bias=True)

    def _make_layer(self, planes: int, blocks: int, mom: float) -> nn.Sequential:
        """resnet.py:86-127: the first block changes the width (with a ``downsample`` when it does), the others keep it."""
        first = (UNetBasicBlock(self.inplanes, planes, mom, self.fused) if self.inplanes != planes
                 else HRBasicBlock(planes, planes, mom, self.fused))
        self.inplanes = planes
        return nn.Sequential(first, *[HRBasicBlock(planes, planes, mom, self.fused) for _ in range(1, blocks)])

    @staticmethod
    def _blocks(seq: nn.Sequential, parts, s1: KernelMap, one: KernelMap, trace: Optional[dict], name: str) -> torch.Tensor:
        first = seq[0]
        if isinstance(first, UNetBasicBlock):
            x = first(parts, s1, one, trace, f"{name}.0.")
        else:
            x = first(parts[0] if len(parts) == 1 else torch.cat(list(parts), dim=1), s1, trace, f"{name}.0.")
        for i, blk in enumerate(list(seq)[1:], 1):
            x = blk(x, s1, trace, f"{name}.{i}.")
        return x

    def _pyramid(self, where) -> UNetPyramid:
        if isinstance(where, UNetPyramid):
            return where
        if isinstance(where, VoxelPyramid):
            where = where.coords[0]
        return build_unet_pyramid(where, self.conv1_kernel_size)

    def forward(self, batch, trace: Optional[dict] = None) -> torch.Tensor:
        where, feats = batch
        pyr = self._pyramid(where)
        if not feats.is_cuda:
            raise _lib.CsnError(_NO_CPU)
        if pyr.coords[0].device != feats.device:
            pyr = pyr.to(feats.device)
        f, tr = self.fused, self.training
        if tuning.current().eval_epilogue and f and not tr and not torch.is_grad_enabled():
            return self._forward_infer(feats, pyr, trace)
        out_p1 = _keep(trace, "bn0", _combine([_conv_bn(self.conv0p1s1, self.bn0, feats, pyr.stem, f)], f, tr, self.bn0.eps))
        skips, out = [out_p1], out_p1
        tail = f and tr and tuning.current().unet_fused_tail           # the resolution changes on the fused nodes (section 26)
        for n, ts in ((1, 1), (2, 2), (3, 4), (4, 8)):
            out = _keep(trace, f"bn{n}", _octant_bn_relu(getattr(self, f"conv{n}p{ts}s2"), getattr(self, f"bn{n}"), out, pyr.oct[n - 1], tail))
            out = self._blocks(getattr(self, f"block{n}"), [out], pyr.s1[n], pyr.one[n], trace, f"block{n}")
            skips.append(out)
        skips.pop()                                                    # block4's output goes up, not across
        for n, ts in ((4, 16), (5, 8), (6, 4), (7, 2)):
            level = 7 - n
            out = _keep(trace, f"bntr{n}", _octant_bn_relu(getattr(self, f"convtr{n}p{ts}s2"), getattr(self, f"bntr{n}"), out, pyr.oct[level],
                                                       tail))
            out = self._blocks(getattr(self, f"block{n + 1}"), [out, skips.pop()], pyr.s1[level], pyr.one[level], trace,
                               f"block{n + 1}")
        return self.final(out)

    @staticmethod
    def _blocks_infer(seq: nn.Sequential, x: torch.Tensor, widths, s1: KernelMap, one: KernelMap, trace: Optional[dict], name: str,
                      out: Optional[torch.Tensor], dtype: Optional[torch.dtype] = None,
                      out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """``_blocks`` on the inference launches; the list's last launch writes ``out`` when given.  ``dtype`` (16-bit maps): the
        type of every map but the list's result, which is ``out``'s own or ``out_dtype``."""
        blocks = list(seq)
        for i, blk in enumerate(blocks):
            last = i == len(blocks) - 1
            to = out if last else None
            od = None if to is not None else (out_dtype if last else dtype)
            if isinstance(blk, UNetBasicBlock):
                x = blk.infer(x, s1, one, trace, f"{name}.{i}.", out=to, widths=widths, dtype=dtype, out_dtype=od)
            else:
                x = blk.infer(x, s1, trace, f"{name}.{i}.", out=to, dtype=dtype, out_dtype=od)
        return x

    def _forward_infer(self, feats: torch.Tensor, pyr: UNetPyramid, trace: Optional[dict]) -> torch.Tensor:
        """The same network with one library call per convolution + norm: ``sparse_conv_bn_act`` for the stem and the blocks
        (``HRBasicBlock.infer`` / ``UNetBasicBlock.infer``), ``octant_conv_bn_act`` for the eight resolution changes.  Every ReLU
        output is a stored map.  Decoder level l's ``[up | skip]`` input is ONE (n_l, P[n] + skip) buffer, allocated before the
        encoder runs: the launch that produces the skip map (``bn0``; the last launch of ``block1`` .. ``block3``) writes its
        columns [P[n], P[n] + skip), the transposed convolution its columns [0, P[n]) and the decoder block reads the buffer through
        its row pitch — no concatenation is ever copied.  Where the buffer would pass the kernels' 2 GiB window the two maps stay
        separate and are joined with ``torch.cat``.  A block that reads more than 256 columns runs ``conv1`` and the
        ``downsample`` convolution as two launches over the buffer's two column blocks, ``(z_up s + t) + z_skip s``: a summation
        order of its own (``UNetBasicBlock.infer``).  ``final`` stays the ``nn.Linear``.

        In math mode "bf16" / "fp16" with ``tuning.rows_single_product``: ``tuning.octant_single_product`` hands the eight
        resolution changes to section 25 (one 16-bit product) on the same fp32 maps; ``tuning.unet_maps16`` does that and makes
        every stored map — the ``[up | skip]`` buffers included, their window sized in their own bytes — a tensor of the mode's
        16-bit type (sections 24 and 25).  The stem's input and the last block's output, which ``final`` reads, stay fp32."""
        P, dev = self.PLANES, feats.device
        t16 = maps16_dtype()
        d = t16 if tuning.current().unet_maps16 else None              # the type of a stored map; None: fp32 maps, today's calls
        sp = t16 is not None and (tuning.current().octant_single_product or tuning.current().unet_maps16)
        esz, last_dtype = (4, None) if d is None else (2, torch.float32)
        od = lambda to: None if to is not None else d                  # the out_dtype of a launch that writes ``to``
        skip_w = (self.INIT_DIM, P[0], P[1], P[2])                     # the skip map's width at level 0 .. 3
        up_w = (P[7], P[6], P[5], P[4])                                # the transposed convolution's at level 0 .. 3
        cat = []
        for l in range(4):
            n_l, w = pyr.coords[l].shape[0], up_w[l] + skip_w[l]
            cat.append(torch.empty((n_l, w), device=dev, dtype=d or torch.float32) if n_l * w * esz <= _mh._WINDOW else None)
        skip_to = lambda l: None if l > 3 or cat[l] is None else cat[l][:, up_w[l]:]
        out = _keep(trace, "bn0", _conv_bn_act(self.conv0p1s1, self.bn0, feats, pyr.stem, out=skip_to(0), out_dtype=od(skip_to(0))))
        skips = [out]
        for n, ts in ((1, 1), (2, 2), (3, 4), (4, 8)):
            out = _keep(trace, f"bn{n}", _octant_bn_act(getattr(self, f"conv{n}p{ts}s2"), getattr(self, f"bn{n}"), out, pyr.oct[n - 1],
                                                        out_dtype=d, single_product=sp))
            out = self._blocks_infer(getattr(self, f"block{n}"), out, None, pyr.s1[n], pyr.one[n], trace, f"block{n}", skip_to(n), d, d)
            skips.append(out)
        skips.pop()                                                    # block4's output goes up, not across
        for n, ts in ((4, 16), (5, 8), (6, 4), (7, 2)):
            l = 7 - n
            up_to = None if cat[l] is None else cat[l][:, :up_w[l]]
            up = _keep(trace, f"bntr{n}", _octant_bn_act(getattr(self, f"convtr{n}p{ts}s2"), getattr(self, f"bntr{n}"), out, pyr.oct[l],
                                                         out=up_to, out_dtype=od(up_to), single_product=sp))
            skip = skips.pop()
            x = cat[l] if cat[l] is not None else torch.cat([up, skip], dim=1)
            out = self._blocks_infer(getattr(self, f"block{n + 1}"), x, (up_w[l], skip_w[l]), pyr.s1[l], pyr.one[l], trace,
                                     f"block{n + 1}", None, d, last_dtype if n == 7 else d)
        return self.final(out)


class Res16UNet14(Res16UNetBase):
    LAYERS = (1, 1, 1, 1, 1, 1, 1, 1)


class Res16UNet18(Res16UNetBase):
    LAYERS = (2, 2, 2, 2, 2, 2, 2, 2)


class Res16UNet34(Res16UNetBase):
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)


class Res16UNet50(Res16UNetBase):
    BLOCK = "Bottleneck"
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)


class Res16UNet101(Res16UNetBase):
    BLOCK = "Bottleneck"
    LAYERS = (2, 3, 4, 23, 2, 2, 2, 2)


class Res16UNet14A(Res16UNet14):
    PLANES = (32, 64, 128, 256, 128, 128, 96, 96)


class Res16UNet14A2(Res16UNet14A):
    LAYERS = (1, 1, 1, 1, 2, 2, 2, 2)


class Res16UNet14B(Res16UNet14):
    PLANES = (32, 64, 128, 256, 128, 128, 128, 128)


class Res16UNet14B2(Res16UNet14B):
    LAYERS = (1, 1, 1, 1, 2, 2, 2, 2)


class Res16UNet14B3(Res16UNet14B):
    LAYERS = (2, 2, 2, 2, 1, 1, 1, 1)


class Res16UNet14C(Res16UNet14):
    PLANES = (32, 64, 128, 256, 192, 192, 128, 128)


class Res16UNet14D(Res16UNet14):
    PLANES = (32, 64, 128, 256, 384, 384, 384, 384)


class Res16UNet18A(Res16UNet18):
    PLANES = (32, 64, 128, 256, 128, 128, 96, 96)


class Res16UNet18B(Res16UNet18):
    PLANES = (32, 64, 128, 256, 128, 128, 128, 128)


class Res16UNet18D(Res16UNet18):
    PLANES = (32, 64, 128, 256, 384, 384, 384, 384)


class Res16UNet34A(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 64, 64)


class Res16UNet34B(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 64, 32)


class Res16UNet34C(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 96, 96)


SUPPORTED = ("Res16UNet14", "Res16UNet14A", "Res16UNet14A2", "Res16UNet14B", "Res16UNet14B2", "Res16UNet14B3", "Res16UNet14C",
             "Res16UNet18", "Res16UNet18A", "Res16UNet18B", "Res16UNet34", "Res16UNet34A", "Res16UNet34B", "Res16UNet34C")
REFUSED = ("Res16UNet14D", "Res16UNet18D", "Res16UNet50", "Res16UNet101")


def load_me_unet_state(model: Res16UNetBase, state_dict) -> Res16UNetBase:
    """Copy a ``Res16UNet`` checkpoint of the reference into ``model``.  The modules keep the reference's names; a
    ``MinkowskiBatchNorm`` wraps its norm, so ``<name>.bn.weight`` etc. map to ``<name>.weight`` (``bnX.bn.*``,
    ``blockN.i.norm1.bn.*``, ``blockN.i.downsample.1.bn.*``); a convolution's ``<name>.kernel`` is (KV, c_in, c_out) on both sides;
    ``final.kernel`` — (c_in, c_out) or (1, c_in, c_out) — is transposed into the ``nn.Linear`` weight and ``final.bias`` — (c_out,)
    or (1, c_out) — flattened.  A missing key or a wrong shape raises ``ValueError`` before the model is touched.  The order of the KV
    axis (the offset and octant numbering of minkowski_conv.py) is this project's choice: parity unpinned against MinkowskiEngine."""
    new = {}
    c_out, c_in = model.final.weight.shape
    for need in ("final.kernel", "final.bias"):
        if need not in state_dict:
            raise ValueError(f"checkpoint has no {need}")
    kernel, bias = state_dict["final.kernel"], state_dict["final.bias"]
    if tuple(kernel.shape) == (1, c_in, c_out):
        kernel = kernel[0]
    if tuple(kernel.shape) != (c_in, c_out):
        raise ValueError(f"final.kernel is {tuple(kernel.shape)}; expected ({c_in}, {c_out}) or (1, {c_in}, {c_out})")
    if tuple(bias.shape) == (1, c_out):
        bias = bias[0]
    if tuple(bias.shape) != (c_out,):
        raise ValueError(f"final.bias is {tuple(bias.shape)}; expected ({c_out},) or (1, {c_out})")
    new["final.weight"], new["final.bias"] = kernel.t(), bias
    for name, mod in model.named_modules():
        if isinstance(mod, (SparseConv3d, SparseConvDown2, CatConv3d)):
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
            if v.dim() == 2 and cur.dim() == 3 and cur.shape[0] == 1:      # a kernel-1 convolution kept as (c_in, c_out)
                v = v[None]
            if tuple(v.shape) != tuple(cur.shape):
                raise ValueError(f"{ref} is {tuple(v.shape)}; expected {tuple(cur.shape)}")
            new[own] = v
    model.load_state_dict(new, strict=True)
    return model
