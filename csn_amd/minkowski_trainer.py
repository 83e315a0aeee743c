"""The MinkowskiNet training procedures: epochs of ``train_iter``, validation, the patience-driven rebuilds of the shape graph,
checkpoints and resume (``CSNTrainer``); the same loop without a graph for the ``HRNetSeg`` baseline (``SegTrainer``); and test mode
for both model families (``test_split``).

Reference (marios2019/CSN):
  * ``Trainer.__init__`` / ``train``: the epoch loop, patience, cooldown, graph rebuilds     MinkowskiNet/lib/trainer_csn.py:20-186
  * ``_construct_shape_graph``                                                             MinkowskiNet/lib/trainer_csn.py:262-282
  * ``_save_curr_checkpoint`` / ``_save_best_checkpoints`` / ``_resume``                    MinkowskiNet/lib/trainer_csn.py:315-387
  * ``checkpoint`` (file names, dictionary keys, the ``weights.pth`` link)                  MinkowskiNet/lib/utils.py:11-61
  * ``InfSampler``                                                                         MinkowskiNet/lib/dataloader.py:5-34
  * the baseline's ``Trainer`` (no graph, no patience, no accumulation)                    MinkowskiNet/lib/trainer_seg.py:18-260
  * test mode: ``is_train = False``                 MinkowskiNet/tasks/main_csn.py:121-141, tasks/main_seg.py:124-130, trainer_csn.py:400-500

Everything on the device is what exists already: a batch is ``PointCollection.batch`` / ``neighbor_batches`` /
``PointBatch.field()``, an iteration is ``train_iter``, validation is ``evaluate``, the graph is ``construct_shape_graph``.  This
module is the host side around them.  The loss and the score of an iteration stay device tensors and are added into a device
accumulator; they are read at ``stat_freq`` and at the end of an epoch, never per iteration.  The reference empties torch's
allocator cache after every iteration (:216); nothing here does.

WHAT THE METHOD IS.  The shape graph starts from random pairs (:78-83).  After every epoch the validation Part IoU is compared
with the best so far; while it does not improve, ``cooldown`` runs down first and ``patience`` after it, and at ``patience <= 0``
the best-Part-IoU checkpoint is loaded again and both splits' neighbours are recomputed with its retrieval measure (:134-158) — at
most ``MAX_GRAPH_CONSTRUCTION`` constructions, the first one included.  ``PatienceState`` is that state machine alone.

CHECKPOINTS.  The reference's dictionary and file names (``checkpoint_<model><postfix>.pth``, ``weights.pth`` a link to the current
one) plus one key, ``csn_amd``, with what an exact resume needs and the reference does not save: the scheduler's state, the
``bit_generator.state`` of the augmentation, sampler and graph generators, the sampler's permutation and position, the iteration
counter as it stands, and the state of torch's CPU generator — the head's dropout masks are counter-based and take their seeds from
it (``csn_amd.functional.draw_seeds``).  A checkpoint without the key loads as the reference's does (``_resume``, :348-387): a
fresh schedule at ``iteration + 1``, fresh generators — a valid continuation, not a bit-equal one.  ``SegTrainer`` writes the same
dictionary without ``csn_data`` and without the graph generator.

The run time of ``test_split`` and the trainers' overhead over a bare ``train_iter`` loop are not measured.
"""
from __future__ import annotations

import dataclasses
import json
import logging
import math
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .minkowski_csn import construct_shape_graph, random_neighbors
from .minkowski_hrnet import HRNetSimCSN, load_me_hrnet_state, load_me_seg_state
from .minkowski_unet import Res16UNetBase, load_me_unet_state
from .minkowski_points import AugmentSpec, PointCollection
from .minkowski_solvers import TrainConfig, initialize_optimizer, initialize_scheduler
from .minkowski_training import evaluate, train_iter

log = logging.getLogger(__name__)

MAX_PATIENCE, MAX_COOLDOWN, MAX_GRAPH_CONSTRUCTION = 10, 5, 3          # trainer_csn.py:36
LR_FACTOR = 0.5                                                        # ReduceLROnPlateau's factor (:41)
Neighbors = List[Tuple[int, List[int]]]


class InfSampler:
    """An endless permutation sampler (dataloader.py:5-34): ``next()`` walks a permutation of ``range(n)`` and draws a fresh one from
    ``rng`` (the caller's ``numpy.random.Generator``) when it is used up; ``shuffle=False`` walks ``0 .. n-1`` over and over.
    ``len()`` is n.  ``state_dict()`` holds the permutation, the position in it and the generator's state."""

    def __init__(self, n: int, shuffle: bool = True, rng: Optional[np.random.Generator] = None):
        if n < 1:
            raise ValueError("InfSampler needs at least one item")
        if shuffle and rng is None:
            raise ValueError("a shuffling InfSampler needs an explicit numpy Generator (rng)")
        self.n, self.shuffle, self.rng = int(n), bool(shuffle), rng
        self._perm: List[int] = []
        self._pos = 0

    def __len__(self) -> int:
        return self.n

    def __iter__(self):
        return self

    def __next__(self) -> int:
        if self._pos >= len(self._perm):
            self._perm = [int(i) for i in (self.rng.permutation(self.n) if self.shuffle else range(self.n))]
            self._pos = 0
        self._pos += 1
        return self._perm[self._pos - 1]

    def state_dict(self) -> dict:
        return {"n": self.n, "shuffle": self.shuffle, "perm": list(self._perm), "pos": self._pos,
                "bit_generator": None if self.rng is None else self.rng.bit_generator.state}

    def load_state_dict(self, state: dict) -> None:
        if state["n"] != self.n or state["shuffle"] != self.shuffle:
            raise ValueError(f"the saved sampler walks {state['n']} items (shuffle={state['shuffle']}), this one {self.n} "
                             f"(shuffle={self.shuffle})")
        self._perm, self._pos = [int(i) for i in state["perm"]], int(state["pos"])
        if self.rng is not None and state["bit_generator"] is not None:
            self.rng.bit_generator.state = state["bit_generator"]


class BestValues:
    """The four best validation values and the iterations they were seen at (trainer_seg.py:40-43, 215-231).  ``record_best(...)``
    moves them (trainer_csn.py:330-346), each stamped with the iteration given, calling ``on_best(postfix)`` right after each one
    moved: a checkpoint written there sees the values moved so far, as the reference's files do."""

    def __init__(self):
        self.best_val_part_iou, self.best_val_part_iou_iter = 0, 0
        self.best_val_shape_iou, self.best_val_shape_iou_iter = 0, 0
        self.best_val_loss, self.best_val_loss_iter = float("inf"), 0
        self.best_val_acc, self.best_val_acc_iter = 0, 0

    def record_best(self, val_loss: float, val_score: float, val_part_iou: float, val_shape_iou: float, curr_iter: int,
                    on_best: Optional[Callable[[str], None]] = None) -> List[str]:
        moved = []

        def hit(postfix):
            moved.append(postfix)
            if on_best is not None:
                on_best(postfix)
        if val_part_iou > self.best_val_part_iou:
            self.best_val_part_iou, self.best_val_part_iou_iter = val_part_iou, curr_iter
            hit("best_part_iou")
        if val_shape_iou > self.best_val_shape_iou:
            self.best_val_shape_iou, self.best_val_shape_iou_iter = val_shape_iou, curr_iter
            hit("best_shape_iou")
        if val_loss < self.best_val_loss:
            self.best_val_loss, self.best_val_loss_iter = val_loss, curr_iter
            hit("best_loss")
        if val_score > self.best_val_acc:
            self.best_val_acc, self.best_val_acc_iter = val_score, curr_iter
            hit("best_acc")
        return moved

    def best_values(self) -> Dict[str, float]:
        return {k: getattr(self, k) for k in ("best_val_part_iou", "best_val_part_iou_iter", "best_val_shape_iou",
                                              "best_val_shape_iou_iter", "best_val_loss", "best_val_loss_iter", "best_val_acc",
                                              "best_val_acc_iter")}


class PatienceState(BestValues):
    """The trainer's state machine (trainer_csn.py:36-52, 114-158), host numbers only.

    ``observe(part_iou)`` is the end of an epoch BEFORE the best values move (:115-130): ``cooldown -= 1``; a Part IoU above the best
    so far resets ``patience``; otherwise — only while ``k_neighbors > 0`` and fewer than ``MAX_GRAPH_CONSTRUCTION`` graphs were built
    — a cooldown that reached zero is held there and ``patience`` falls by one.  ``record_best(...)`` then moves the four best values
    (``BestValues``).  ``should_rebuild()``: ``k_neighbors > 0`` and ``patience <= 0``
    (:134-136).  ``rebuilt()``: one more construction, patience and cooldown back at their maxima (:154-156); ``constructed()`` is
    the first, random graph, which only counts (:82)."""

    def __init__(self, k_neighbors: int):
        super().__init__()
        self.k_neighbors = int(k_neighbors)
        self.patience, self.cooldown = MAX_PATIENCE, MAX_COOLDOWN
        self.n_graph_construction = 0

    def observe(self, val_part_iou: float) -> None:
        self.cooldown -= 1
        if val_part_iou > self.best_val_part_iou:
            self.patience = MAX_PATIENCE
        elif self.k_neighbors > 0 and self.n_graph_construction < MAX_GRAPH_CONSTRUCTION:
            if self.cooldown <= 0:
                self.cooldown = 0
                self.patience -= 1

    def should_rebuild(self) -> bool:
        return self.k_neighbors > 0 and self.patience <= 0

    def constructed(self) -> None:
        self.n_graph_construction += 1

    def rebuilt(self) -> None:
        self.n_graph_construction += 1
        self.patience, self.cooldown = MAX_PATIENCE, MAX_COOLDOWN


# ------------------------------------------------------------------------------------------------------
# what the two trainers and test mode share
# ------------------------------------------------------------------------------------------------------
def load_model_state(model, state_dict) -> None:
    """A checkpoint's ``state_dict`` in either layout: this project's names (``backbone.*`` with ``head.*`` / ``final.*``; a
    ``Res16UNet``'s ``final.weight``) go through ``load_state_dict``; any other dictionary is taken for the reference's layout and
    goes through ``load_me_hrnet_state`` (an ``HRNetSimCSN``), ``load_me_unet_state`` (a ``Res16UNet``) or ``load_me_seg_state`` (an
    ``HRNetSeg``)."""
    if any(k.startswith("backbone.") for k in state_dict) or (isinstance(model, Res16UNetBase) and "final.weight" in state_dict):
        model.load_state_dict(state_dict)
    elif isinstance(model, HRNetSimCSN):
        load_me_hrnet_state(model, state_dict)
    elif isinstance(model, Res16UNetBase):
        load_me_unet_state(model, state_dict)
    else:
        load_me_seg_state(model, state_dict)


def checkpoint_num_labels(state_dict) -> int:
    """The rows of a checkpoint's output layer: ``head.output.weight`` / ``final.3.weight`` / ``final.weight`` (out, in) here, the
    last axis of ``output.kernel`` / ``final.3.kernel`` / ``final.kernel`` ((1,) in, out) in the reference's layout."""
    for name, axis in (("head.output.weight", 0), ("final.3.weight", 0), ("output.kernel", -1), ("final.3.kernel", -1),
                       ("final.weight", 0), ("final.kernel", -1)):
        if name in state_dict:
            return int(state_dict[name].shape[axis])
    raise ValueError("the checkpoint has no output layer: none of head.output.weight, final.3.weight, output.kernel, final.3.kernel, "
                     "final.weight, final.kernel")


def _model_num_labels(model) -> int:
    if isinstance(model, HRNetSimCSN):
        return int(model.head.output.out_features)
    return int((model.final if isinstance(model, Res16UNetBase) else model.final[3]).out_features)


def _forward(model, batch):
    """``forward_fn`` of ``train_iter`` / ``evaluate`` for a ``(queries_field, key_fields)`` batch: the logits interpolated onto the
    queries' points, and their offsets.  An ``HRNetSeg`` takes no keys."""
    field, keys = batch
    if isinstance(model, HRNetSimCSN):
        return field.interpolate(model(field.sparse(), [k.sparse() for k in keys] or None)), field.offsets
    return field.interpolate(model(field.sparse())), field.offsets


def _collate(queries_from: PointCollection, keys_from: Optional[PointCollection], q_idx: Sequence[int], neighbors: Optional[Neighbors],
             K: int, params, voxel_size: float, shift, quantization_mode: str):
    """``((queries_field, key_fields), target)`` for the shapes ``q_idx`` of ``queries_from`` and, with ``K > 0``, the i-th neighbour
    of every one of them from ``keys_from``; ``params`` (None: unaugmented) holds ``(K + 1) * len(q_idx)`` items, the queries' first."""
    B = len(q_idx)
    queries = queries_from.batch(q_idx, None if params is None else params.slice(0, B), voxel_size, shift)
    keys = []
    if K > 0:
        keys = keys_from.neighbor_batches([neighbors[int(i)] for i in q_idx], K,
                                          None if params is None else params.slice(B, (K + 1) * B), voxel_size, shift)
    return (queries.field(quantization_mode), [k.field(quantization_mode) for k in keys]), queries.labels


def _in_order(n_shapes: int, batch_size: int):
    for lo in range(0, n_shapes, batch_size):
        yield list(range(lo, min(lo + batch_size, n_shapes)))


def _backbone_shapes(model, col: PointCollection, batch_size: int, voxel_size: float, quantization_mode: str) -> List[torch.Tensor]:
    """The backbone rows of every shape of ``col`` (unaugmented, no grad): what ``construct_shape_graph`` scores.  All of them
    stay resident until the graph is built: voxels x backbone channels x 4 bytes per split."""
    out = []
    with torch.no_grad():
        for idx in _in_order(col.n_shapes, batch_size):
            rows, off = model.backbone_rows(col.batch(idx, None, voxel_size).field(quantization_mode).sparse())
            off = [int(v) for v in off.tolist()]
            out += [rows[a:b] for a, b in zip(off, off[1:])]
    return out


class _SubBatches:
    """The ``iter_size`` sub-batches of one iteration, fetched one at a time as ``train_iter`` walks them (it asks for ``len()``
    first): one sub-batch is resident at a time, as in trainer_csn.py:194-210."""

    def __init__(self, trainer: "_Trainer"):
        self.trainer = trainer
        self.rows = 0

    def __len__(self) -> int:
        return self.trainer.cfg.iter_size

    def __iter__(self):
        t = self.trainer
        for _ in range(t.cfg.iter_size):
            batch, target = t.fetch([next(t.sampler) for _ in range(t.cfg.batch_size)])
            self.rows = int(target.shape[0])
            yield batch, target


class _Trainer:
    """What ``CSNTrainer`` and ``SegTrainer`` share: the batches, one epoch, one validation, the checkpoint files.  A subclass sets
    ``k_neighbors``, ``scheduler`` and ``state`` (a ``BestValues``) and writes ``train()``."""

    k_neighbors = 0
    train_neighbors: Optional[Neighbors] = None
    val_neighbors: Optional[Neighbors] = None

    def __init__(self, model, train_collection: PointCollection, val_collection: PointCollection, cfg: TrainConfig,
                 spec: Optional[AugmentSpec], seed: int, val_batch_size: int, quantization_mode: str):
        if train_collection.labels is None or val_collection.labels is None:
            raise ValueError("both collections need per-point labels")
        if cfg.batch_size < 1 or cfg.iter_size < 1 or val_batch_size < 1:
            raise ValueError("batch_size, iter_size and val_batch_size must be at least 1")
        self.model, self.train_collection, self.val_collection, self.cfg = model, train_collection, val_collection, cfg
        self.spec = AugmentSpec.distort_partnet() if spec is None else spec
        self.val_batch_size, self.quantization_mode = int(val_batch_size), quantization_mode
        self.num_labels = _model_num_labels(model)
        self.aug_rng, sampler_rng = (np.random.default_rng([int(seed), i]) for i in range(2))
        self.sampler = InfSampler(train_collection.n_shapes, True, sampler_rng)
        self.optimizer = initialize_optimizer(model.parameters(), cfg)
        self.curr_iter, self.epoch = 1, 1                                         # trainer_csn.py:51, trainer_seg.py:44

    # ---- batches ----
    def _forward(self, batch):
        return _forward(self.model, batch)

    def _fields(self, queries_from: PointCollection, q_idx: Sequence[int], neighbors: Optional[Neighbors], augment: bool):
        K = self.k_neighbors
        if K > 0 and neighbors is None:
            raise ValueError("no shape graph yet: call construct_graphs() or load a checkpoint that holds one")
        p = self.spec.draw((K + 1) * len(q_idx), self.aug_rng) if augment else None
        return _collate(queries_from, self.train_collection, q_idx, neighbors, K, p, self.cfg.voxel_size, self.spec.shift,
                        self.quantization_mode)

    def fetch(self, q_idx: Sequence[int]):
        """``_fetch_data`` (trainer_csn.py:236-260, trainer_seg.py:166-175) for the training shapes ``q_idx``: ``((queries_field,
        key_fields), target)`` — the queries and the i-th neighbour of every query (none for an ``HRNetSeg``), each item augmented
        with numbers of its own from the augmentation generator."""
        return self._fields(self.train_collection, q_idx, self.train_neighbors, True)

    def _val_batches(self):
        for idx in _in_order(self.val_collection.n_shapes, self.val_batch_size):
            yield self._fields(self.val_collection, idx, self.val_neighbors, False)

    # ---- one epoch, one validation ----
    @property
    def iters_per_epoch(self) -> int:
        return math.ceil(len(self.sampler) / self.cfg.batch_size / self.cfg.iter_size)

    def _plateau(self) -> bool:
        return self.cfg.scheduler == "ReduceLROnPlateau"

    def train_epoch(self) -> Tuple[float, float]:
        """``iters_per_epoch`` iterations of ``train_iter`` (trainer_csn.py:94-103, trainer_seg.py:68-77), ``iter_size`` sub-batches
        each; the scheduler steps per iteration unless it is ``ReduceLROnPlateau``.  Returns the epoch's (loss, score) averages,
        weighted as the reference's meters are (trainer_csn.py:223-224: by the rows of the last sub-batch) — the epoch's one read
        besides those at ``stat_freq``."""
        cfg = self.cfg
        self.model.train()
        acc, rows = None, 0
        n_iter = self.iters_per_epoch
        for _ in range(n_iter):
            subs = _SubBatches(self)
            loss, score = train_iter(self._forward, subs, self.optimizer, None if self._plateau() else self.scheduler, cfg.ignore_label)
            term = torch.stack([loss.double(), score.double()]) * subs.rows
            acc = term if acc is None else acc + term
            rows += subs.rows
            if self.curr_iter % cfg.stat_freq == 0 or self.curr_iter == 1:
                l, s = (acc / rows).tolist()
                log.info("===> Epoch[%d](%d/%d): Loss %.4f\tLR: %.3e\tScore %.3f", self.epoch, self.curr_iter, n_iter, l, self.lr, s)
            self.curr_iter += 1
        l, s = (acc / rows).tolist()
        return l, s

    @property
    def lr(self) -> float:
        return self.optimizer.param_groups[0]["lr"]

    def validate(self) -> Tuple[float, float, float, float]:
        """``_validate`` / ``Trainer.test`` (trainer_csn.py:226-234, 400-500; trainer_seg.py:157-164, 272-356) through ``evaluate``:
        (loss, precision, Part IoU, Shape IoU) of the validation split in eval mode; the mode it found is restored."""
        was_training = self.model.training
        self.model.eval()
        try:
            return evaluate(self._forward, self._val_batches(), self.num_labels, self.cfg.ignore_label)
        finally:
            self.model.train(was_training)

    def _record(self, val, save_current: bool = False) -> None:
        loss, score, part_iou, shape_iou = val
        if save_current:
            self._save_curr_checkpoint()
        self.state.record_best(loss, score, part_iou, shape_iou, self.curr_iter, on_best=self._save_curr_checkpoint)
        st = self.state
        log.info("Validation at iter %d: loss %.3f, score %.3f, Part IoU %.3f, Shape IoU %.3f", self.curr_iter, loss, score, part_iou, shape_iou)
        log.info("Current best Part IoU: %.3f at iter %d", st.best_val_part_iou, st.best_val_part_iou_iter)
        log.info("Current best Shape IoU: %.3f at iter %d", st.best_val_shape_iou, st.best_val_shape_iou_iter)
        log.info("Current best Loss: %.3f at iter %d", st.best_val_loss, st.best_val_loss_iter)
        log.info("Current best Score: %.3f at iter %d", st.best_val_acc, st.best_val_acc_iter)

    # ---- checkpoints ----
    def checkpoint_path(self, postfix: Optional[str] = None) -> str:
        return os.path.join(self.cfg.log_dir, f"checkpoint_{self.cfg.model}{postfix or ''}.pth")

    def checkpoint_state(self) -> dict:
        """The dictionary ``save_checkpoint`` writes: the reference's keys (utils.py:25-51) and ``csn_amd``."""
        state = {"iteration": self.curr_iter, "epoch": self.epoch + 1, "arch": self.cfg.model, "state_dict": self.model.state_dict(),
                 "optimizer": self.optimizer.state_dict()}
        state.update(self.state.best_values())
        state["csn_amd"] = {"version": 1, "curr_iter": self.curr_iter, "scheduler": self.scheduler.state_dict(),
                            "augment_rng": self.aug_rng.bit_generator.state, "sampler": self.sampler.state_dict(),
                            "torch_rng_state": torch.get_rng_state()}
        return state

    def save_checkpoint(self, path: str) -> None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.checkpoint_state(), path)
        log.info("Checkpoint saved to %s", path)

    def _save_curr_checkpoint(self, postfix: Optional[str] = None) -> None:
        path = self.checkpoint_path(postfix)
        self.save_checkpoint(path)
        if postfix is None:                                                      # utils.py:52-61: the settings, and weights.pth -> the file
            with open(os.path.join(self.cfg.log_dir, "config.json"), "w") as fh:
                json.dump(dataclasses.asdict(self.cfg), fh, indent=4)
            link = os.path.join(self.cfg.log_dir, "weights.pth")
            if os.path.lexists(link):
                os.remove(link)
            os.symlink(os.path.basename(path), link)

    def _load_model_state(self, state_dict) -> None:
        load_model_state(self.model, state_dict)

    def load_checkpoint(self, path: str) -> dict:
        """``_resume`` (trainer_csn.py:348-387, trainer_seg.py:233-259).  With the ``csn_amd`` key the run continues bit for bit
        (given ``resume_optimizer``); without it, as the reference resumes.  Returns the dictionary read."""
        if not os.path.isfile(path):
            raise ValueError(f"no checkpoint found at '{path}'")
        log.info("=> Loading checkpoint '%s'", path)
        state = torch.load(path, map_location="cpu")
        extra = state.get("csn_amd")
        self.curr_iter = int(extra["curr_iter"]) if extra else int(state["iteration"]) + 1
        self.epoch = int(state["epoch"])
        self._load_model_state(state["state_dict"])
        if self.cfg.resume_optimizer:
            if extra:
                self.optimizer.load_state_dict(state["optimizer"])
                self.scheduler.load_state_dict(extra["scheduler"])
            else:
                self.scheduler = initialize_scheduler(self.optimizer, self.cfg, last_step=self.curr_iter, factor=LR_FACTOR)
                self.optimizer.load_state_dict(state["optimizer"])
        for k in self.state.best_values():
            if k in state:
                setattr(self.state, k, state[k])
        if extra:
            self.aug_rng.bit_generator.state = extra["augment_rng"]
            self.sampler.load_state_dict(extra["sampler"])
            torch.set_rng_state(extra["torch_rng_state"])
        log.info("=> Loaded checkpoint '%s' (epoch %d)", path, self.epoch)
        return state


class CSNTrainer(_Trainer):
    """``Trainer`` of trainer_csn.py for an ``HRNetSimCSN`` on two resident ``PointCollection``s (both normalised by the caller, both
    with labels, on the model's device).  ``cfg`` is a ``TrainConfig``; ``spec`` the training augmentation (None:
    ``AugmentSpec.distort_partnet()``); ``seed`` seeds the three generators the trainer owns — augmentation, sampler, random graph.
    The dropout seeds come from torch's CPU generator: ``torch.manual_seed`` before the run fixes them.  Validation walks the
    validation split in order, ``val_batch_size`` shapes at a time (config.py: 1), unaugmented, keys from the TRAINING split."""

    def __init__(self, model, train_collection: PointCollection, val_collection: PointCollection, cfg: TrainConfig,
                 spec: Optional[AugmentSpec] = None, seed: int = 0, val_batch_size: int = 1,
                 quantization_mode: str = "random_subsample"):
        if cfg.k_neighbors < 0 or cfg.k_neighbors > train_collection.n_shapes - 1:
            raise ValueError(f"k_neighbors must lie in [0, {train_collection.n_shapes - 1}] for {train_collection.n_shapes} training shapes")
        if cfg.k_neighbors > 0 and model.head.k_neighbors == 0:
            raise ValueError("the model's head was built with k_neighbors = 0: it takes no key batches")
        super().__init__(model, train_collection, val_collection, cfg, spec, seed, val_batch_size, quantization_mode)
        self.k_neighbors = cfg.k_neighbors
        self.graph_rng = np.random.default_rng([int(seed), 2])
        self.scheduler = initialize_scheduler(self.optimizer, cfg, factor=LR_FACTOR, patience=MAX_PATIENCE, cooldown=MAX_COOLDOWN * 2)
        self.state = PatienceState(cfg.k_neighbors)

    # ---- the shape graph ----
    def _backbone_shapes(self, col: PointCollection) -> List[torch.Tensor]:
        return _backbone_shapes(self.model, col, self.cfg.batch_size, self.cfg.voxel_size, self.quantization_mode)

    def construct_graphs(self, recalculate: bool = False) -> None:
        """``_construct_shape_graph`` (:262-282) in eval mode (the mode it found is restored): the first construction pairs every
        shape with random training shapes (``construct_shape_graph``'s random branch, from the graph generator), a recalculation
        ranks the training shapes by the model's retrieval measure — for the training split among themselves, never a shape
        itself, for the validation split against the training split."""
        K = self.cfg.k_neighbors
        if K < 1:
            raise ValueError("k_neighbors = 0: there is no shape graph")
        was_training = self.model.training
        self.model.eval()
        try:
            log.info("===> %s shape graph for the training and validation splits", "Recalculate" if recalculate else "Construct")
            if recalculate:
                train_rows, val_rows = self._backbone_shapes(self.train_collection), self._backbone_shapes(self.val_collection)
                self.train_neighbors = construct_shape_graph(self.model.head, train_rows, None, K)
                self.val_neighbors = construct_shape_graph(self.model.head, val_rows, train_rows, K)
            else:
                n_train, n_val = self.train_collection.n_shapes, self.val_collection.n_shapes
                self.train_neighbors = random_neighbors(n_train, n_train, K, True, self.graph_rng)
                self.val_neighbors = random_neighbors(n_val, n_train, K, False, self.graph_rng)
        finally:
            self.model.train(was_training)

    # ---- the procedure ----
    def train(self) -> None:
        """``Trainer.train`` (:54-186)."""
        cfg, st = self.cfg, self.state
        self.model.train()
        log.info("===> Start training")
        if cfg.resume:
            self.load_checkpoint(os.path.join(cfg.resume, "weights.pth"))
            if st.should_rebuild():                                              # the run stopped between the verdict and the rebuild
                self.construct_graphs(recalculate=True)
                st.rebuilt()
        elif cfg.k_neighbors > 0:
            self.construct_graphs(recalculate=False)
            st.constructed()
        while True:
            self.train_epoch()
            if self.epoch >= cfg.max_epoch:
                break
            self._save_curr_checkpoint()                                         # before the validation, as the reference does
            val = self.validate()
            st.observe(val[2])
            log.info("=====> (Iteration:%d) patience %d, cooldown %d", self.curr_iter, st.patience, st.cooldown)
            self._record(val)
            if st.should_rebuild():
                self._reload_best()
                self.construct_graphs(recalculate=True)
                st.rebuilt()
                self._save_curr_checkpoint()                                     # keeps the new graph
            self.model.train()
            if self._plateau():
                self.scheduler.step(val[0])
            self.epoch += 1
        self._record(self.validate(), save_current=True)

    def _reload_best(self) -> None:
        """:136-148: back to the best-Part-IoU weights before the graph is recomputed; with ``resume_optimizer`` its optimizer too,
        the rate back at ``cfg.lr`` and a fresh schedule that starts at the current iteration."""
        path = self.checkpoint_path("best_part_iou")
        log.info("=====> Loading checkpoint '%s'", path)
        state = torch.load(path, map_location="cpu")
        self._load_model_state(state["state_dict"])
        log.info("=====> Checkpoint loaded from epoch %s (iter %s)", state["epoch"], state["iteration"])
        if self.cfg.resume_optimizer:
            self.optimizer.load_state_dict(state["optimizer"])
            for group in self.optimizer.param_groups:
                group["lr"] = group["initial_lr"] = self.cfg.lr
            self.scheduler = initialize_scheduler(self.optimizer, self.cfg, last_step=self.curr_iter, factor=LR_FACTOR)

    # ---- checkpoints ----
    def checkpoint_state(self) -> dict:
        """The shared dictionary, ``csn_data`` (trainer_csn.py:315-328; only with ``k_neighbors > 0``) and the graph generator."""
        st = self.state
        state = super().checkpoint_state()
        if self.cfg.k_neighbors > 0:
            state["csn_data"] = {"patience": st.patience, "cooldown": st.cooldown, "n_graph_construction": st.n_graph_construction,
                                 "train_neighbors": self.train_neighbors, "val_neighbors": self.val_neighbors}
        state["csn_amd"]["graph_rng"] = self.graph_rng.bit_generator.state
        return state

    def load_checkpoint(self, path: str) -> dict:
        state = super().load_checkpoint(path)
        st = self.state
        if "csn_data" in state:
            data = state["csn_data"]
            st.patience, st.cooldown, st.n_graph_construction = int(data["patience"]), int(data["cooldown"]), int(data["n_graph_construction"])
            self.train_neighbors = [(int(q), [int(i) for i in nb]) for q, nb in data["train_neighbors"]]
            self.val_neighbors = [(int(q), [int(i) for i in nb]) for q, nb in data["val_neighbors"]]
            log.info("===> Patience=%d, Cooldown=%d, #Graph construction=%d", st.patience, st.cooldown, st.n_graph_construction)
        if state.get("csn_amd"):
            self.graph_rng.bit_generator.state = state["csn_amd"]["graph_rng"]
        return state


class SegTrainer(_Trainer):
    """``Trainer`` of trainer_seg.py:18-260 for an ``HRNetSeg`` on two resident, labelled ``PointCollection``s: the baseline cross-shape
    attention is measured against.  The arguments are ``CSNTrainer``'s; ``cfg.k_neighbors`` is ignored (there are no key batches, no
    graph, no patience), and ``cfg.iter_size != 1`` raises — trainer_seg.py has no gradient accumulation and would silently ignore
    the setting.  ``seed`` seeds the augmentation and sampler generators, the same streams a ``CSNTrainer`` of that seed draws from."""

    def __init__(self, model, train_collection: PointCollection, val_collection: PointCollection, cfg: TrainConfig,
                 spec: Optional[AugmentSpec] = None, seed: int = 0, val_batch_size: int = 1,
                 quantization_mode: str = "random_subsample"):
        if cfg.iter_size != 1:
            raise ValueError(f"iter_size = {cfg.iter_size}: the HRNetSeg procedure has no gradient accumulation (trainer_seg.py:121-155)")
        super().__init__(model, train_collection, val_collection, cfg, spec, seed, val_batch_size, quantization_mode)
        self.scheduler = initialize_scheduler(self.optimizer, cfg, factor=LR_FACTOR)            # trainer_seg.py:35-37
        self.state = BestValues()

    def train(self) -> None:
        """``Trainer.train`` (trainer_seg.py:46-119): the last epoch ends without a checkpoint or a validation of its own (:80-83);
        the final validation, the current checkpoint and the best files follow the loop (:115-117)."""
        cfg = self.cfg
        self.model.train()
        log.info("===> Start training")
        if cfg.resume:
            self.load_checkpoint(os.path.join(cfg.resume, "weights.pth"))
        while True:
            self.train_epoch()
            if self.epoch >= cfg.max_epoch:
                break
            self._save_curr_checkpoint()                                         # before the validation, as the reference does
            val = self.validate()
            self._record(val)
            self.model.train()
            if self._plateau():
                self.scheduler.step(val[0])
            self.epoch += 1
        self._record(self.validate(), save_current=True)


# ------------------------------------------------------------------------------------------------------
# test mode
# ------------------------------------------------------------------------------------------------------
RESULTS_LOG = "results_log.txt"


def test_split(model, test_collection: PointCollection, *, train_collection: Optional[PointCollection] = None, k_neighbors: int = 0,
               voxel_size: float = 0.05, ignore_label: int = 255, test_batch_size: int = 1,
               quantization_mode: str = "random_subsample", save_pred_dir: Optional[str] = None,
               screen: Optional[bool] = None) -> Tuple[float, float, float, float]:
    """``Trainer.test`` with ``is_train = False`` (trainer_csn.py:400-500, trainer_seg.py:272-356) and the graph construction in front
    of it (main_csn.py:121-137), for an ``HRNetSimCSN`` or an ``HRNetSeg``: (loss, precision, Part IoU, Shape IoU) of the labelled
    ``test_collection``, walked in order, unaugmented, ``test_batch_size`` shapes at a time (the last batch may be short), in eval
    mode under ``no_grad``; the mode found is restored, parameters and buffers are untouched.

    An ``HRNetSeg``, or ``k_neighbors == 0``, uses no neighbours.  An ``HRNetSimCSN`` with ``k_neighbors > 0`` needs
    ``train_collection``: every test shape's neighbours are ranked among the TRAINING shapes by the model's retrieval measure on
    the unaugmented backbone rows of both splits, as ``CSNTrainer.construct_graphs(recalculate=True)`` ranks the validation split —
    never random, and no index is excluded (the splits differ).  ``screen`` goes to ``construct_shape_graph``.

    ``save_pred_dir`` (None: nothing is written) is created if missing and receives ``results_log.txt`` — ``"Shape IoU: <x>\\nPart
    IoU: <y>"``, both rounded with ``np.round(., 2)``, no trailing newline (trainer_csn.py:492-496) — which
    ``csn_amd.collect_partnet_results`` gathers.

    Two deliberate differences.  A directory that already holds an entry raises ``ValueError`` BEFORE any device work; the reference
    raises the same error only after it has built the graph (trainer_csn.py:431-435 runs after main_csn.py:130).  Scoring is per
    shape (``evaluate(per_shape=True)``) at any ``test_batch_size``; the reference scores a batch as one shape (trainer_csn.py:474),
    which is the same thing at its default ``test_batch_size = 1``."""
    if save_pred_dir is not None:
        os.makedirs(save_pred_dir, exist_ok=True)
        if os.listdir(save_pred_dir):
            raise ValueError(f"Directory {save_pred_dir} not empty. Please remove the existing prediction.")
    if test_collection.labels is None:
        raise ValueError("the test collection needs per-point labels")
    if test_batch_size < 1 or k_neighbors < 0:
        raise ValueError("test_batch_size must be at least 1 and k_neighbors at least 0")
    K = int(k_neighbors) if isinstance(model, HRNetSimCSN) else 0
    if K > 0 and train_collection is None:
        raise ValueError(f"k_neighbors = {K}: the neighbours of the test shapes are training shapes, so train_collection is needed")
    was_training = model.training
    model.eval()
    try:
        log.info("===> Start testing")
        neighbors = None
        if K > 0:
            log.info("===> Construct shape graph for test split")
            test_rows = _backbone_shapes(model, test_collection, test_batch_size, voxel_size, quantization_mode)
            train_rows = _backbone_shapes(model, train_collection, test_batch_size, voxel_size, quantization_mode)
            neighbors = construct_shape_graph(model.head, test_rows, train_rows, K, screen=screen)
            del test_rows, train_rows
        batches = (_collate(test_collection, train_collection, idx, neighbors, K, None, voxel_size, AugmentSpec().shift, quantization_mode)
                   for idx in _in_order(test_collection.n_shapes, test_batch_size))
        loss, score, part_iou, shape_iou = evaluate(lambda batch: _forward(model, batch), batches, _model_num_labels(model), ignore_label)
    finally:
        model.train(was_training)
    if save_pred_dir is not None:
        with open(os.path.join(save_pred_dir, RESULTS_LOG), "w") as fh:
            fh.write("Shape IoU: " + str(np.round(shape_iou, 2)) + "\nPart IoU: " + str(np.round(part_iou, 2)))
    return loss, score, part_iou, shape_iou


test_split.__test__ = False                 # a public name, not a test: pytest must not collect it where it is imported
