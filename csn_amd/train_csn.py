#!/usr/bin/env python3
"""Train an ``HRNetSimCSN`` with the patience-driven shape-graph procedure, or test one: what MinkowskiNet/tasks/main_csn.py does, on
``csn_amd.minkowski_trainer.CSNTrainer`` and ``test_split``.

    python -m csn_amd.train_csn --log_dir <out> --model HRNetSimCSN3S --k_neighbors 1 --lr 0.05 --optimizer SGD --batch_size 8
                                --scheduler ReduceLROnPlateau --max_epoch 200
                                --data_root <sem_seg_h5/Category-3> --train_files train-00.h5 ... --val_files val-00.h5 ...
    python -m csn_amd.train_csn --is_train False --weights <out>/weights.pth --log_dir <out>/evaluation --model HRNetSimCSN3S
                                --k_neighbors 1 --data_root <...> --train_files train-00.h5 ... --test_files test-00.h5 ...

* Every field of ``TrainConfig`` is an argument of its name with config.py's default; of what scripts/train_csn.sh passes these are
  ``--log_dir --model --k_neighbors --lr --optimizer --batch_size --scheduler --max_epoch``.  Its ``--dataset``,
  ``--partnet_category``, ``--train_limit_numpoints`` and ``--input_feat`` select a dataset class the reference resolves itself; here
  the files are named (``--data_root``, ``--train_files``, ``--val_files``, ``--test_files``, read by
  ``PointCollection.from_h5_files``) and any argument not listed by ``--help`` is an error.
* ``--normalize_coords`` / ``--normalize_method``, ``--distort_partnet``, ``--avg_feat``, ``--d_model``, ``--n_head``, ``--seed``,
  ``--val_batch_size``, ``--test_batch_size``: config.py's names and defaults.  ``--num_labels`` is the dataset class's
  ``NUM_LABELS`` (default: the largest training label + 1; in test mode the rows of the checkpoint's output layer).
* ``--weights <file>`` (config.py: ``"None"``) loads the file's ``state_dict``, in this project's layout or the reference's, before
  training or testing (main_csn.py:108-115).
* ``--is_train False`` (scripts/test_csn.sh) is test mode: it needs ``--weights`` and ``--test_files`` — with ``--k_neighbors > 0``
  also ``--train_files``, whose shapes the neighbours are; ``--val_files`` is not needed.  It ranks the test split against the training
  split, evaluates it, logs the four "Test split" lines of main_csn.py:138-141 and writes ``<save_pred_dir>/results_log.txt``
  (``--save_pred_dir``, default ``<log_dir>/results``; it must be empty), which ``python -m csn_amd.collect_partnet_results`` gathers.
* ``--synthetic N`` needs no files: N training and ceil(N / 2) validation shapes, each 150-260 points on an ellipsoid shell,
  labelled 1..8 by octant; in test mode ceil(N / 2) further shapes are the test split.
* ``--resume <log_dir>`` continues from ``<log_dir>/weights.pth``.
"""
import argparse
import dataclasses
import logging
import os
import sys

from .minkowski_solvers import OPTIMIZERS, SCHEDULERS, TrainConfig

MODELS = ("HRNetSimCSN2S", "HRNetSimCSN3S")
SYNTHETIC_LABELS = 9                          # label 0 is never predicted (trainer_csn.py:221): the octants are 1..8
CSN_ONLY = ("k_neighbors", "d_model", "n_head")

log = logging.getLogger(__name__)


def _bool(v: str) -> bool:
    return v.lower() in ("true", "1")        # config.py:14-15


def build_parser(prog: str = "python -m csn_amd.train_csn", models=MODELS, doc: str = __doc__, csn: bool = True) -> argparse.ArgumentParser:
    """The parser of ``train_csn``; ``csn=False`` is ``train_seg``'s: the same arguments without ``CSN_ONLY``."""
    ap = argparse.ArgumentParser(prog=prog, description=doc.split("\n\n")[0], allow_abbrev=False)
    choices = {"optimizer": OPTIMIZERS, "scheduler": SCHEDULERS, "model": models}
    for f in dataclasses.fields(TrainConfig):
        if not csn and f.name in CSN_ONLY:
            continue
        kind = {"bool": _bool, "int": int, "float": float}.get(f.type if isinstance(f.type, str) else f.type.__name__, str)
        default = models[-1] if f.name == "model" else f.default
        ap.add_argument(f"--{f.name}", type=kind, default=default, choices=choices.get(f.name))
    ap.add_argument("--data_root", type=str, default="")
    ap.add_argument("--train_files", type=str, nargs="+", default=None)
    ap.add_argument("--val_files", type=str, nargs="+", default=None)
    ap.add_argument("--test_files", type=str, nargs="+", default=None)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="use N generated ellipsoid shells instead of files")
    ap.add_argument("--num_labels", type=int, default=None)
    ap.add_argument("--normalize_coords", type=_bool, default=False)
    ap.add_argument("--normalize_method", type=str, default="sphere", choices=("sphere", "box"))
    ap.add_argument("--distort_partnet", type=_bool, default=False)
    ap.add_argument("--avg_feat", type=_bool, default=False)
    if csn:
        ap.add_argument("--d_model", type=int, default=256)
        ap.add_argument("--n_head", type=int, default=4)
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--is_train", type=_bool, default=True, help="False: test mode")
    ap.add_argument("--weights", type=str, default="None", help="a checkpoint whose state_dict is loaded first")
    ap.add_argument("--save_pred_dir", type=str, default=None, help="test mode: where results_log.txt goes (default <log_dir>/results)")
    ap.add_argument("--val_batch_size", type=int, default=1)
    ap.add_argument("--test_batch_size", type=int, default=1)
    return ap


def parse_args(argv=None, ap=None):
    """(TrainConfig, the remaining arguments).  Exits with status 2 on an unknown argument or an unusable combination."""
    ap = build_parser() if ap is None else ap
    args = ap.parse_args(argv)
    k_neighbors = getattr(args, "k_neighbors", 0)
    if args.val_batch_size < 1 or args.test_batch_size < 1:
        ap.error("--val_batch_size and --test_batch_size must be at least 1")
    if args.synthetic:
        if args.synthetic < 2 or args.train_files or args.val_files or args.test_files:
            ap.error("--synthetic N needs N >= 2 and takes no --train_files / --val_files / --test_files")
    elif not args.is_train:
        if not args.test_files:
            ap.error("test mode: name the data: --test_files (under --data_root), or --synthetic N")
        if k_neighbors > 0 and not args.train_files:
            ap.error("test mode with --k_neighbors > 0 ranks the test shapes against the training shapes: name --train_files")
    elif not (args.train_files and args.val_files):
        ap.error("name the data: --train_files and --val_files (under --data_root), or --synthetic N")
    if not args.is_train and args.weights.lower() == "none":
        ap.error("--is_train False needs --weights <checkpoint>")
    cfg = TrainConfig(**{f.name: getattr(args, f.name, 0) for f in dataclasses.fields(TrainConfig)})      # train_seg has no k_neighbors: 0
    return cfg, args


def synthetic_shapes(n: int, seed: int, lo: int = 150, hi: int = 260):
    """n shapes for a run without data: between ``lo`` and ``hi`` points (counts differ) on an ellipsoid shell with random semi-axes
    in [0.4, 1], as float32 ``(n_i, 3)`` arrays, and their labels 1..8 by octant as int32 ``(n_i,)`` arrays.  The first m shapes of
    a longer draw with the same seed are the m shapes of a shorter one."""
    import numpy as np
    rng = np.random.default_rng([int(seed), 77])
    points, labels = [], []
    for i in range(n):
        count = lo + (i * 41 + int(rng.integers(0, 7))) % (hi - lo + 1)
        d = rng.standard_normal((count, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = (d * rng.uniform(0.4, 1.0, size=3)).astype(np.float32)
        points.append(p)
        labels.append((1 + (p[:, 0] > 0) + 2 * (p[:, 1] > 0) + 4 * (p[:, 2] > 0)).astype(np.int32))
    return points, labels


def synthetic_split_sizes(n: int, test_mode: bool):
    """``--synthetic N``: (train, validation, test) shape counts, consecutive slices of one ``synthetic_shapes`` draw."""
    half = (n + 1) // 2
    return n, half, half if test_mode else 0


def run(cfg: TrainConfig, args, csn: bool) -> int:
    """What follows the argument parsing, for both command lines (main_csn.py:47-141, main_seg.py:44-130)."""
    logging.basicConfig(format="%(asctime)s -- %(name)s -- %(message)s", datefmt="%d/%m/%Y %H:%M:%S", level=logging.INFO,
                        handlers=[logging.StreamHandler(sys.stdout)])
    import torch

    from . import minkowski_hrnet, minkowski_unet
    from .minkowski_points import AugmentSpec, PointCollection
    from .minkowski_trainer import CSNTrainer, SegTrainer, checkpoint_num_labels, load_model_state, test_split

    if not torch.cuda.is_available():
        raise SystemExit(f"{'train_csn' if csn else 'train_seg'}: no GPU found (there is no CPU path)")
    torch.manual_seed(args.seed)                                                  # main_csn.py:47; the dropout seeds follow it
    test_mode, K = not args.is_train, cfg.k_neighbors if csn else 0
    need = {"train": args.is_train or K > 0, "val": args.is_train, "test": test_mode}
    if args.synthetic:
        pts, labs = synthetic_shapes(sum(synthetic_split_sizes(args.synthetic, test_mode)), args.seed)
        n_train, n_val, _ = synthetic_split_sizes(args.synthetic, test_mode)
        bounds = {"train": (0, n_train), "val": (n_train, n_train + n_val), "test": (n_train + n_val, len(pts))}
        splits = {k: PointCollection(pts[lo:hi], labs[lo:hi]) for k, (lo, hi) in bounds.items() if need[k]}
    else:
        files = {"train": args.train_files, "val": args.val_files, "test": args.test_files}
        splits = {k: PointCollection.from_h5_files(files[k], args.data_root) for k in files if need[k]}
    if args.normalize_coords:
        for col in splits.values():
            col.normalize(args.normalize_method)

    state = None
    if args.weights.lower() != "none":
        log.info("===> Loading weights: %s", args.weights)
        state = torch.load(args.weights, map_location="cpu")
    if args.num_labels:
        num_labels = args.num_labels
    elif test_mode:
        num_labels = checkpoint_num_labels(state["state_dict"])
    else:
        num_labels = SYNTHETIC_LABELS if args.synthetic else int(splits["train"].labels.max()) + 1
    net = getattr(minkowski_hrnet, cfg.model, None) or getattr(minkowski_unet, cfg.model)
    model = net(3, num_labels, d_model=args.d_model, n_head=args.n_head, k_neighbors=K) if csn else net(3, num_labels)
    model = model.to("cuda")
    if state is not None:
        load_model_state(model, state["state_dict"])
    mode = "unweighted_average" if args.avg_feat else "random_subsample"

    if test_mode:
        save_pred_dir = args.save_pred_dir or os.path.join(cfg.log_dir, "results")
        loss, score, part_iou, shape_iou = test_split(model, splits["test"], train_collection=splits.get("train"), k_neighbors=K,
                                                      voxel_size=cfg.voxel_size, ignore_label=cfg.ignore_label,
                                                      test_batch_size=args.test_batch_size, quantization_mode=mode,
                                                      save_pred_dir=save_pred_dir)
        at = f"at iter {state.get('iteration', 0)}" + (f" (K={K})" if csn else "")
        log.info("Test split Part IOU: %.3f %s", part_iou, at)
        log.info("Test split Shape IOU: %.3f %s", shape_iou, at)
        log.info("Test split Loss: %.3f %s", loss, at)
        log.info("Test Score: %.3f %s", score, at)
        return 0
    spec = AugmentSpec.distort_partnet() if args.distort_partnet else AugmentSpec()
    trainer = (CSNTrainer if csn else SegTrainer)(model, splits["train"], splits["val"], cfg, spec=spec, seed=args.seed,
                                                  val_batch_size=args.val_batch_size, quantization_mode=mode)
    trainer.train()
    return 0


def main(argv=None) -> int:
    cfg, args = parse_args(argv)
    return run(cfg, args, csn=True)


if __name__ == "__main__":
    sys.exit(main())
