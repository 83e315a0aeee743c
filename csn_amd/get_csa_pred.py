#!/usr/bin/env python3
"""The test mode of the MID-FC workflow: what ``MID-FC/get_csa_pred.py`` means to be and, as written, is not (``csa_dataset``
and ``args.weight_decay`` are never defined, :188-193; ``validate_layers`` is called with 5 arguments for 6, :117; the per-point
predictions of :137 are never written).

Loads ``<logs_dir>/trained_layers.pth`` into ``get_model(attention_type, num_classes, n_heads, K)``, runs the test split once
in eval mode and writes the Part IoU: the reference's lines appended to ``<logs_dir>/logs.txt`` and
``<logs_dir>/part_IoU_summaries.csv`` in the layout ``DataFrame([[v]], columns=[part]).to_csv`` gives (:196-200).

Command line = what the launcher builds (run_csa_pred.py:67-78), nothing more is required::

    python get_csa_pred.py --logs_dir=<logs>/pretrained_models/run_1/<Part> --knn_graphs=<logs>/pretrained_models/knn_graphs/n_heads_H/<Part>
                           --num_workers=W --batch_size=B --partname=<Part> --num_classes=C --attention_type=csa --n_heads=H --K=K

* ``--knn_graphs`` is the DIRECTORY holding ``test.npy``, as the launcher passes it (the reference reads a hard-coded path
  instead, :182).
* The feature files are found as in ``save_knn_graph``: ``--dataroot`` or the environment variable ``CSN_DATAROOT``.
* ``csa`` types read ``CSADatasetK(test_root, train_root, test_graph, K)`` (csa_training.py:298); ``ssa`` types read
  ``FeaturesDataset(test_root)`` and need no graph.
* ``--batch_size`` is taken, as the launcher passes it; the test loader reads one shape per batch whatever it says, as the
  reference's does (:188, csa_training.py:299).
* ``--testing`` (:29, :151-152) stops after the first batch.
* ``--save_pred_dir`` writes every shape's per-point predictions to ``<dir>/<name>.npy`` (int64, the shape's own points: the
  length of its label file, before the wrap-around padding).
"""
import argparse
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from .save_knn_graph import DATAROOT_ENV, split_root

SUMMARY_NAME = "part_IoU_summaries.csv"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--logs_dir", type=str, required=True, help="directory holding trained_layers.pth; logs.txt and the summary go here")
    ap.add_argument("--knn_graphs", type=str, default=None, help="directory holding test.npy (csa types)")
    ap.add_argument("--dataroot", type=str, default=None, help=f"feature root (default: ${DATAROOT_ENV})")
    ap.add_argument("--num_workers", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--partname", type=str, required=True)
    ap.add_argument("--num_classes", type=int, required=True)
    ap.add_argument("--attention_type", type=str, default="csa")
    ap.add_argument("--n_heads", type=int, default=8)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--testing", action="store_true")
    ap.add_argument("--save_pred_dir", type=str, default=None)
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    args = build_parser().parse_args(argv)
    if args.dataroot is None:
        args.dataroot = os.environ.get(DATAROOT_ENV)
    return args


def logprint(log: str, logs_fp=None) -> None:
    """get_csa_pred.py:45-49: print, and append to the log file when one is given."""
    if logs_fp is not None:
        with open(logs_fp, "a") as f:
            f.write(log + "\n")
    print(log)


def write_summary(path: str, partname: str, value: float) -> None:
    """The bytes of ``pd.DataFrame([[value]], columns=[partname]).to_csv(path)`` (:196-200): an empty index header, one row
    with index 0, the float in its shortest round-trip form."""
    with open(path, "w", newline="") as f:
        f.write(f",{partname}\n0,{float(value)!r}\n")


def shape_names(dataset) -> list:
    """(file name, own points) per shape of a FeaturesDataset / CSADatasetK, in item order: the own points are the length of
    the label file (the header alone is read)."""
    own = getattr(dataset, "own", dataset)
    return [(name, int(np.load(os.path.join(own.labels_dir, name), mmap_mode="r").shape[0])) for name in own.files]


def main(argv=None):
    args = parse_args(argv)
    if not args.dataroot:
        raise SystemExit(f"get_csa_pred: no data root — pass --dataroot or set {DATAROOT_ENV} (the reference hard-codes "
                         "its cluster path, get_csa_pred.py:171)")

    from .csa_models import get_model
    from .data import CSADatasetK, FeaturesDataset
    from .training import test_layers

    os.makedirs(args.logs_dir, exist_ok=True)
    logs_fp = os.path.join(args.logs_dir, "logs.txt")
    device = torch.device("cuda")
    logprint(f"device:{device}")

    model = get_model(args.attention_type, args.num_classes, args.n_heads, args.K).to(device)
    model_path = os.path.join(args.logs_dir, "trained_layers.pth")
    model.load_state_dict(torch.load(model_path, map_location="cpu"))
    logprint(f"model wts loaded from {model_path}!", logs_fp)

    test_root = split_root(args.dataroot, "test", args.partname)
    if args.attention_type.startswith("csa"):
        if not args.knn_graphs:
            raise SystemExit("get_csa_pred: --knn_graphs (the directory holding test.npy) is needed for a csa model")
        test_graph = np.load(os.path.join(args.knn_graphs, "test.npy"))
        print("test graph:", test_graph.shape)
        dataset = CSADatasetK(test_root, split_root(args.dataroot, "train", args.partname), test_graph, args.K)
    else:
        dataset = FeaturesDataset(test_root)
    loader = DataLoader(dataset, 1, shuffle=False, num_workers=args.num_workers)      # one shape per batch, as at :188

    logprint("---- Validation ----", logs_fp)
    res = test_layers(model, loader, args.num_classes, device, names=shape_names(dataset) if args.save_pred_dir else None,
                      save_pred_dir=args.save_pred_dir, max_batches=1 if args.testing else None)
    logprint(f"Final shape_IoU: {res['part_iou'] * 100}", logs_fp)      # (:194 — the reference's label for its Part IoU)
    logprint(f"loss: {res['loss']}, accuracy: {res['accuracy']}, shape IoU over {res['shapes']} shapes: {res['shape_iou'] * 100}", logs_fp)

    df_path = os.path.join(args.logs_dir, SUMMARY_NAME)
    write_summary(df_path, args.partname, res["part_iou"] * 100)
    logprint(f"test IoU saved to {df_path}", logs_fp)
    return res


if __name__ == "__main__":
    main()
