"""Everything between the MinkowskiNet head's logits and ``optimizer.step()`` / the two reported metrics, on the MI355X.

Reference (marios2019/CSN):
  * ``Trainer._train_iter``          MinkowskiNet/lib/trainer_csn.py:188-224
  * ``Trainer.test``                 MinkowskiNet/lib/trainer_csn.py:400-500
  * ``precision_at_one_partnet``     MinkowskiNet/lib/utils.py:64-75
  * ``calculate_iou`` / ``calculate_shape_iou`` / ``calculate_part_iou``     MinkowskiNet/lib/utils.py:78-176
  * ``AverageMeter``                 MinkowskiNet/lib/utils.py:228-244
  * ``get_neighbors``                MinkowskiNet/lib/csn_utils.py:114-130

The reference pulls targets and predictions to the host every iteration (``loss.item()``, ``.cpu().numpy()``, the per-label
Python loop of ``calculate_iou``).  Here ``seg_loss`` is ONE pass over the point-major logits (``csn_ragged_seg_fwd_f32``: the
cross-entropy with ``ignore_index``, the prediction ``1 + argmax over classes 1..``, the precision's sums and the per-(shape,
label) counts the IoUs derive from) and one pass for the gradient (``csn_ragged_seg_bwd_f32``); ``SegMeter`` accumulates on the
device and synchronises once, in ``result()``.

The MID-FC loss path (csn_amd/training.py, ``csn_masked_ce_*``) is a different loss on a different layout and is untouched.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from . import functional as CF
from .minkowski_csn import Ragged, SimCSNHead, _host_offsets, _int32_pair


class SegBatch(NamedTuple):
    """What one ``seg_loss`` call leaves for the metrics, as DEVICE tensors (nothing is read back):
    ``pred`` (N,) int32 = 1 + argmax over classes 1..; ``stats`` (4,) float64 = mean loss, counted rows, correct rows, bad rows;
    ``counts`` (S, n_classes, 3) int32 = per segment and label: intersection, ground-truth, prediction counts."""
    pred: torch.Tensor
    stats: torch.Tensor
    counts: torch.Tensor


class _SegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, off_pair, ignore_label):
        L = _lib.lib()
        N, n_cls = logits.shape
        dev = logits.device
        oh, od = off_pair
        S = oh.numel() - 1
        lse = torch.empty((N,), device=dev, dtype=torch.float32)
        nll = torch.empty((N,), device=dev, dtype=torch.float32)
        pred = torch.empty((N,), device=dev, dtype=torch.int32)
        stats = torch.empty((4,), device=dev, dtype=torch.float64)
        counts = torch.empty((S, n_cls, 3), device=dev, dtype=torch.int32)
        ws_bytes = int(L.csn_ragged_seg_workspace_bytes(N))
        ws = torch.empty((ws_bytes // 8,), device=dev, dtype=torch.float64)
        _lib.check(L.csn_ragged_seg_fwd_f32(CF._ptr(logits), N, logits.stride(0), CF._ptr(target), oh.data_ptr(), CF._ptr(od), S, n_cls,
                                            int(ignore_label), CF._ptr(lse), CF._ptr(nll), CF._ptr(pred), CF._ptr(stats), CF._ptr(counts), CF._ptr(ws),
                                            ws_bytes, CF._stream()), "csn_ragged_seg_fwd_f32")
        ctx.save_for_backward(logits, target, lse, nll, stats)
        ctx.ignore_label = int(ignore_label)
        ctx.mark_non_differentiable(pred, stats, counts)
        return stats[0].float(), pred, stats, counts

    @staticmethod
    def backward(ctx, grad_loss, _gp, _gs, _gc):
        logits, target, lse, nll, stats = ctx.saved_tensors
        N, n_cls = logits.shape
        g = grad_loss.detach().float().reshape(1).contiguous()
        dlogits = torch.empty((N, n_cls), device=logits.device, dtype=torch.float32)
        _lib.check(_lib.lib().csn_ragged_seg_bwd_f32(CF._ptr(logits), N, logits.stride(0), CF._ptr(target), n_cls, ctx.ignore_label,
                                                     CF._ptr(lse), CF._ptr(nll), CF._ptr(stats), CF._ptr(g), CF._ptr(dlogits), n_cls,
                                                     CF._stream()),
                   "csn_ragged_seg_bwd_f32")
        return dlogits, None, None, None


def seg_loss(logits: torch.Tensor, target: torch.Tensor, offsets=None, ignore_label: int = 255) -> Tuple[torch.Tensor, SegBatch]:
    """``nn.CrossEntropyLoss(ignore_index=ignore_label)(logits, target)`` (trainer_csn.py:205, :471) as a 0-dim fp32 tensor with
    its gradient, and the ``SegBatch`` of the same pass.  ``logits`` (N, n_classes) fp32 point-major rows on the device (any row
    pitch, columns contiguous), ``target`` (N,) integer labels on the device, ``offsets`` (S + 1) the rows of each shape (None:
    the whole batch is one segment, as trainer_csn.py:474 scores it).  No row counted gives nan, as torch does.  A label that
    is neither ``ignore_label`` nor in [0, n_classes) enters nothing but ``stats[3]``; ``SegMeter.result()`` raises for it."""
    if not (logits.is_cuda and target.is_cuda):
        raise _lib.CsnError("csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    CF._need_cuda(logits)
    if logits.dim() != 2 or logits.shape[1] < 2 or logits.shape[0] < 1:
        raise ValueError("logits must be (N >= 1, n_classes >= 2) point-major rows")
    if target.dim() != 1 or target.shape[0] != logits.shape[0] or target.is_floating_point():
        raise ValueError("target must be (N,) integer labels, one per row of the logits")
    N = logits.shape[0]
    if logits.stride(1) != 1 or (N > 1 and logits.stride(0) < logits.shape[1]):
        logits = logits.contiguous()
    target = target.long().contiguous()
    off = _host_offsets([0, N] if offsets is None else offsets, N)
    loss, pred, stats, counts = _SegLoss.apply(logits, target, _int32_pair(off, logits.device), int(ignore_label))
    return loss, SegBatch(pred, stats, counts)


def precision(seg_batch: SegBatch) -> torch.Tensor:
    """``precision_at_one_partnet`` (utils.py:64-75) of a batch, 0..100, as a 0-dim device tensor (nan with no counted row)."""
    return seg_batch.stats[2] * 100.0 / seg_batch.stats[1]


class SegMeter:
    """The bookkeeping of ``Trainer.test`` (trainer_csn.py:407, 472-475, 488-500) without a host synchronisation per batch:
    ``update`` adds a batch's sums into device tensors (int64 counts, float64 sums), ``result`` reads them back once and
    finishes ``losses.avg``, ``scores.avg``, ``calculate_part_iou`` and ``calculate_shape_iou`` (both x 100)."""

    def __init__(self, num_labels: int):
        if num_labels < 2:
            raise ValueError("num_labels must be >= 2")
        self.num_labels = int(num_labels)
        self._state = None

    def _init(self, dev):
        z = lambda n, dt: torch.zeros((n,), device=dev, dtype=dt)
        # inter / union per label; [shape IoU sum]; [shapes with a present label]; [loss x rows, precision x rows, bad rows]; rows
        self._state = {"inter": z(self.num_labels, torch.int64), "union": z(self.num_labels, torch.int64),
                       "shape_iou": z(1, torch.float64), "shapes": z(1, torch.int64), "sums": z(3, torch.float64)}
        self._rows = 0

    def update(self, seg_batch: SegBatch, n_rows: int) -> None:
        """``ious[iteration] = calculate_iou(...)`` for every segment of the batch, ``losses.update(loss, n_rows)`` and
        ``scores.update(precision, n_rows)`` — on the device the batch lives on."""
        counts, stats = seg_batch.counts, seg_batch.stats
        if counts.dim() != 3 or counts.shape[1] != self.num_labels or counts.shape[2] != 3:
            raise ValueError(f"counts must be (segments, {self.num_labels}, 3)")
        if self._state is None:
            self._init(counts.device)
        st = self._state
        c = counts.long()
        inter = c[:, :, 0]
        union = c[:, :, 1] + c[:, :, 2] - inter
        st["inter"] += inter.sum(dim=0)
        st["union"] += union.sum(dim=0)
        # calculate_iou keeps a label of a shape iff its union > 0 (labels 1..); calculate_shape_iou averages the kept ones and
        # skips a shape that kept none
        present = union[:, 1:] > 0
        iou = torch.where(present, inter[:, 1:].double() / union[:, 1:].clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=c.device))
        kept = present.sum(dim=1)
        per_shape = iou.sum(dim=1) / kept.clamp(min=1).double()
        st["shape_iou"] += torch.where(kept > 0, per_shape, torch.zeros_like(per_shape)).sum()
        st["shapes"] += (kept > 0).sum()
        s = stats.double()
        st["sums"] += torch.stack([s[0] * n_rows, s[2] * 100.0 / s[1] * n_rows, s[3]])
        self._rows += int(n_rows)

    def result(self) -> Tuple[float, float, float, float]:
        """(losses.avg, scores.avg, Part IoU, Shape IoU): the one synchronisation.  Raises ValueError if any row had a label that
        is neither the ignore label nor a class (torch's loss raises for it at once)."""
        if self._state is None:
            raise ValueError("no batch was added")
        st = self._state
        flat = torch.cat([st["inter"].double(), st["union"].double(), st["shape_iou"], st["shapes"].double(), st["sums"]]).cpu().tolist()
        n = self.num_labels
        inter, union = flat[:n], flat[n:2 * n]
        shape_sum, shapes, loss_sum, score_sum, n_bad = flat[2 * n:2 * n + 5]
        if n_bad > 0:
            raise ValueError(f"{int(n_bad)} target labels are neither the ignore label nor in [0, {n})")
        part = sum((inter[i] / union[i]) if union[i] > 0 else 0.0 for i in range(1, n)) / float(n - 1)
        shape = shape_sum / shapes if shapes > 0 else float("nan")
        return loss_sum / self._rows, score_sum / self._rows, part * 100, shape * 100


Batch = Tuple[object, torch.Tensor]      # (whatever forward_fn takes, target (N,))


def train_iter(forward_fn: Callable, sub_batches: Sequence[Batch], optimizer, scheduler=None, ignore_label: int = 255):
    """``Trainer._train_iter`` (trainer_csn.py:188-224): ``zero_grad``; for every sub-batch ``(batch, target)``
    ``forward_fn(batch) -> (logits, offsets)``, the loss divided by ``iter_size = len(sub_batches)`` and its backward; then ONE
    ``optimizer.step()`` and one ``scheduler.step()``.  Returns (the summed loss, the precision of the LAST sub-batch), as the
    reference feeds its meters (:221-224) — device tensors, nothing is read back."""
    iter_size = len(sub_batches)
    if iter_size < 1:
        raise ValueError("train_iter needs at least one sub-batch")
    optimizer.zero_grad()
    batch_loss, last = None, None
    for batch, target in sub_batches:
        logits, offsets = forward_fn(batch)
        loss, last = seg_loss(logits, target.to(logits.device), offsets, ignore_label)
        loss = loss / iter_size
        batch_loss = loss.detach() if batch_loss is None else batch_loss + loss.detach()
        loss.backward()
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return batch_loss, precision(last)


def evaluate(forward_fn: Callable, batches: Iterable[Batch], num_labels: int, ignore_label: int = 255, per_shape: bool = True):
    """``Trainer.test`` (trainer_csn.py:400-500) under ``no_grad``: every ``(batch, target)`` goes through
    ``forward_fn(batch) -> (logits, offsets)`` and ``seg_loss``; returns ``SegMeter.result()`` = (loss, precision, Part IoU,
    Shape IoU).  ``per_shape=False`` scores each batch as ONE "model", which is what the reference does when a test batch holds
    several shapes (:474).  Train / eval mode is the caller's business, as in ``construct_shape_graph``."""
    meter = SegMeter(num_labels)
    with torch.no_grad():
        for batch, target in batches:
            logits, offsets = forward_fn(batch)
            _, sb = seg_loss(logits, target.to(logits.device), offsets if per_shape else None, ignore_label)
            meter.update(sb, logits.shape[0])
    return meter.result()


def neighbor_batches(key_shapes: Sequence[torch.Tensor], neighbors: Sequence[Tuple[int, Sequence[int]]], K: int) -> List[Ragged]:
    """``get_neighbors`` (csn_utils.py:114-130) on per-shape feature tensors: key batch i is the packed ``(rows, offsets)`` of the
    i-th neighbour of every query, in the queries' order — what ``SimCSNHead.forward(keys=...)`` takes, straight from
    ``construct_shape_graph``'s ``[(q_idx, [neighbours])]``."""
    if K < 1:
        raise ValueError("K must be >= 1")
    out = []
    for i in range(K):
        rows, off = [], [0]
        for _, nbrs in neighbors:
            if len(nbrs) < K:
                raise ValueError(f"every query needs at least K = {K} neighbours")
            t = key_shapes[int(nbrs[i])]
            rows.append(t)
            off.append(off[-1] + int(t.shape[0]))
        out.append((torch.cat(rows), off))
    return out


def load_me_head_state(head: SimCSNHead, state_dict) -> SimCSNHead:
    """Copy the head of an ``HRNetSimCSN`` checkpoint (hrnet.py:341-357) into a ``SimCSNHead``: ``MHA.*`` and ``linear_q/k.weight``
    by name; ``output`` is a kernel-size-1 ``MinkowskiConvolution`` there and an ``nn.Linear`` here, so ``output.kernel`` —
    (2C, out) or (1, 2C, out) — is transposed into ``output.weight`` (out, 2C) and ``output.bias`` — (out,) or (1, out) — is
    flattened.  Any other shape raises.  (The two layouts are MinkowskiEngine's documented ones; no ME tensor was read.)
    A head built with ``backbone_channels`` takes ``fc_layer`` too (hrnet.py:332-339): ``fc_layer.0.kernel`` — (c_in, C) or
    (1, c_in, C) — transposed into ``fc_layer.0.weight``, ``fc_layer.0.bias`` flattened, and the ``fc_layer.1.bn.*`` tensors of the
    MinkowskiBatchNorm wrapper into ``fc_layer.1.*``; a head without it ignores those keys."""
    own = head.state_dict()
    out_ch, two_c = head.output.weight.shape
    new = {}
    for name in own:
        if name.startswith("MHA.") or name in ("linear_q.weight", "linear_k.weight"):
            if name not in state_dict:
                raise ValueError(f"checkpoint has no {name}")
            new[name] = state_dict[name]
    for need in ("output.kernel", "output.bias"):
        if need not in state_dict:
            raise ValueError(f"checkpoint has no {need}")
    kernel, bias = state_dict["output.kernel"], state_dict["output.bias"]
    if tuple(kernel.shape) == (1, two_c, out_ch):
        kernel = kernel[0]
    if tuple(kernel.shape) != (two_c, out_ch):
        raise ValueError(f"output.kernel is {tuple(kernel.shape)}; expected ({two_c}, {out_ch}) or (1, {two_c}, {out_ch})")
    if tuple(bias.shape) == (1, out_ch):
        bias = bias[0]
    if tuple(bias.shape) != (out_ch,):
        raise ValueError(f"output.bias is {tuple(bias.shape)}; expected ({out_ch},) or (1, {out_ch})")
    new["output.weight"] = kernel.t()
    new["output.bias"] = bias
    if getattr(head, "fc_layer", None) is not None:
        C, c_in = head.fc_layer[0].weight.shape
        for need in ("fc_layer.0.kernel", "fc_layer.0.bias"):
            if need not in state_dict:
                raise ValueError(f"checkpoint has no {need}")
        kernel, bias = state_dict["fc_layer.0.kernel"], state_dict["fc_layer.0.bias"]
        if tuple(kernel.shape) == (1, c_in, C):
            kernel = kernel[0]
        if tuple(kernel.shape) != (c_in, C):
            raise ValueError(f"fc_layer.0.kernel is {tuple(kernel.shape)}; expected ({c_in}, {C}) or (1, {c_in}, {C})")
        if tuple(bias.shape) == (1, C):
            bias = bias[0]
        if tuple(bias.shape) != (C,):
            raise ValueError(f"fc_layer.0.bias is {tuple(bias.shape)}; expected ({C},) or (1, {C})")
        new["fc_layer.0.weight"] = kernel.t()
        new["fc_layer.0.bias"] = bias
        for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            if f"fc_layer.1.bn.{leaf}" not in state_dict:
                raise ValueError(f"checkpoint has no fc_layer.1.bn.{leaf}")
            new[f"fc_layer.1.{leaf}"] = state_dict[f"fc_layer.1.bn.{leaf}"]
    with torch.no_grad():
        for name, v in new.items():
            if tuple(own[name].shape) != tuple(v.shape):
                raise ValueError(f"{name} is {tuple(v.shape)}; the head holds {tuple(own[name].shape)}")
        for name, v in new.items():
            own[name].copy_(v)
    return head
