#!/usr/bin/env python3
"""Train an ``HRNetSimCSN`` with the patience-driven shape-graph procedure: what MinkowskiNet/tasks/main_csn.py does with
``is_train``, on ``csn_amd.minkowski_trainer.CSNTrainer``.

    python -m csn_amd.train_csn --log_dir <out> --model HRNetSimCSN3S --k_neighbors 1 --lr 0.05 --optimizer SGD --batch_size 8
                                --scheduler ReduceLROnPlateau --max_epoch 200
                                --data_root <sem_seg_h5/Category-3> --train_files train-00.h5 ... --val_files val-00.h5 ...

* Every field of ``TrainConfig`` is an argument of its name with config.py's default; of what scripts/train_csn.sh passes these are
  ``--log_dir --model --k_neighbors --lr --optimizer --batch_size --scheduler --max_epoch``.  Its ``--dataset``,
  ``--partnet_category``, ``--train_limit_numpoints`` and ``--input_feat`` select a dataset class the reference resolves itself; here
  the files are named (``--data_root``, ``--train_files``, ``--val_files``, read by ``PointCollection.from_h5_files``) and any
  argument not listed by ``--help`` is an error.
* ``--normalize_coords`` / ``--normalize_method``, ``--distort_partnet``, ``--avg_feat``, ``--d_model``, ``--n_head``, ``--seed``: config.py's
  names and defaults.  ``--num_labels`` (default: the largest training label + 1) is the dataset class's ``NUM_LABELS``.
* ``--synthetic N`` needs no files: N training and ceil(N / 2) validation shapes, each 150-260 points on an ellipsoid shell,
  labelled 1..8 by octant.
* ``--resume <log_dir>`` continues from ``<log_dir>/weights.pth``.
"""
import argparse
import dataclasses
import logging
import sys

from .minkowski_solvers import OPTIMIZERS, SCHEDULERS, TrainConfig

MODELS = ("HRNetSimCSN2S", "HRNetSimCSN3S")
SYNTHETIC_LABELS = 9                          # label 0 is never predicted (trainer_csn.py:221): the octants are 1..8


def _bool(v: str) -> bool:
    return v.lower() in ("true", "1")        # config.py:14-15


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m csn_amd.train_csn", description=__doc__.split("\n\n")[0], allow_abbrev=False)
    choices = {"optimizer": OPTIMIZERS, "scheduler": SCHEDULERS, "model": MODELS}
    for f in dataclasses.fields(TrainConfig):
        kind = {"bool": _bool, "int": int, "float": float}.get(f.type if isinstance(f.type, str) else f.type.__name__, str)
        ap.add_argument(f"--{f.name}", type=kind, default=f.default, choices=choices.get(f.name))
    ap.add_argument("--data_root", type=str, default="")
    ap.add_argument("--train_files", type=str, nargs="+", default=None)
    ap.add_argument("--val_files", type=str, nargs="+", default=None)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="train on N generated ellipsoid shells instead of files")
    ap.add_argument("--num_labels", type=int, default=None)
    ap.add_argument("--normalize_coords", type=_bool, default=False)
    ap.add_argument("--normalize_method", type=str, default="sphere", choices=("sphere", "box"))
    ap.add_argument("--distort_partnet", type=_bool, default=False)
    ap.add_argument("--avg_feat", type=_bool, default=False)
    ap.add_argument("--d_model", type=int, default=256)
    ap.add_argument("--n_head", type=int, default=4)
    ap.add_argument("--seed", type=int, default=123)
    return ap


def parse_args(argv=None):
    """(TrainConfig, the remaining arguments).  Exits with status 2 on an unknown argument or an unusable combination."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.synthetic:
        if args.synthetic < 2 or args.train_files or args.val_files:
            ap.error("--synthetic N needs N >= 2 and takes no --train_files / --val_files")
    elif not (args.train_files and args.val_files):
        ap.error("name the data: --train_files and --val_files (under --data_root), or --synthetic N")
    cfg = TrainConfig(**{f.name: getattr(args, f.name) for f in dataclasses.fields(TrainConfig)})
    return cfg, args


def synthetic_shapes(n: int, seed: int, lo: int = 150, hi: int = 260):
    """n shapes for a run without data: between ``lo`` and ``hi`` points (counts differ) on an ellipsoid shell with random semi-axes
    in [0.4, 1], as float32 ``(n_i, 3)`` arrays, and their labels 1..8 by octant as int32 ``(n_i,)`` arrays."""
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


def main(argv=None) -> int:
    cfg, args = parse_args(argv)
    logging.basicConfig(format="%(asctime)s -- %(name)s -- %(message)s", datefmt="%d/%m/%Y %H:%M:%S", level=logging.INFO,
                        handlers=[logging.StreamHandler(sys.stdout)])
    import torch

    from . import minkowski_hrnet
    from .minkowski_points import AugmentSpec, PointCollection
    from .minkowski_trainer import CSNTrainer

    if not torch.cuda.is_available():
        raise SystemExit("train_csn: no GPU found (there is no CPU path)")
    torch.manual_seed(args.seed)                                                  # main_csn.py:47; the dropout seeds follow it
    if args.synthetic:
        pts, labs = synthetic_shapes(args.synthetic + (args.synthetic + 1) // 2, args.seed)
        train = PointCollection(pts[:args.synthetic], labs[:args.synthetic])
        val = PointCollection(pts[args.synthetic:], labs[args.synthetic:])
        num_labels = args.num_labels or SYNTHETIC_LABELS
    else:
        train = PointCollection.from_h5_files(args.train_files, args.data_root)
        val = PointCollection.from_h5_files(args.val_files, args.data_root)
        num_labels = args.num_labels or int(train.labels.max()) + 1
    if args.normalize_coords:
        train.normalize(args.normalize_method)
        val.normalize(args.normalize_method)
    model = getattr(minkowski_hrnet, cfg.model)(3, num_labels, d_model=args.d_model, n_head=args.n_head, k_neighbors=cfg.k_neighbors)
    model = model.to("cuda")
    spec = AugmentSpec.distort_partnet() if args.distort_partnet else AugmentSpec()
    trainer = CSNTrainer(model, train, val, cfg, spec=spec, seed=args.seed,
                         quantization_mode="unweighted_average" if args.avg_feat else "random_subsample")
    trainer.train()
    return 0


if __name__ == "__main__":
    sys.exit(main())
