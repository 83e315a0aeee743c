"""Generate tests/golden/g12_minkowski_seg.npz by running the REFERENCE's own metric functions (MinkowskiNet/lib/utils.py) and
torch's nn.CrossEntropyLoss, as Trainer.test (MinkowskiNet/lib/trainer_csn.py:400-500) strings them together.

Run once, where the reference checkout exists (as for make_golden.py):

    python tests/golden/make_golden_g12.py [reference root]

utils.py imports only json, logging, os, errno, time, numpy and torch, so it is loaded by path (MinkowskiEngine is not needed).
The targets are stored; the logits are regenerated from ``numpy.random.default_rng`` by tests/minkowski_seg_ref.g12_logits, so only
numbers the reference PRODUCED are written.  The reference is imported, never copied.

Every sequence is a run of ragged test batches.  Between them they hold: rows labelled 0, rows labelled 255 (ignored), labels
absent from a shape, a shape whose labels are all 0, exact ties between two classes, and num_labels 4, 15 and 39.
Stored per batch: the loss, precision_at_one_partnet, calculate_iou's intersections and unions per shape (nan where its dicts
have no key) and for the whole batch as one "model" (what trainer_csn.py:474 does); per sequence: losses.avg, scores.avg,
calculate_part_iou x 100, calculate_shape_iou x 100 for both groupings.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")     # a checkout beside this one

spec = importlib.util.spec_from_file_location("ref_utils", os.path.join(REFERENCE, "MinkowskiNet", "lib", "utils.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)  # (the reference)

from tests.minkowski_seg_ref import g12_logits  # noqa: E402

IGNORE = 255

# (num_labels, seed, batches); a batch is a list of shapes; a shape is (rows, labels it may carry, share of 0 rows, share of 255 rows)
SEQUENCES = [
    (4, 1201, [[(57, [1, 2, 3], 0.1, 0.1), (131, [1, 3], 0.2, 0.0)],
               [(64, [2], 0.0, 0.3), (1, [3], 0.0, 0.0), (90, [], 1.0, 0.0)],             # a one-row shape; a shape of 0 labels only
               [(203, [1, 2, 3], 0.05, 0.05)]]),
    (15, 1202, [[(150, list(range(1, 15)), 0.1, 0.1), (77, [3, 4, 9], 0.1, 0.1), (33, [14], 0.5, 0.2)],
                [(40, [], 1.0, 0.0), (260, [1, 2, 5, 7, 11, 13], 0.0, 0.15)]]),
    (39, 1203, [[(301, list(range(1, 39)), 0.1, 0.1)],
                [(120, [5, 6, 7, 30, 38], 0.1, 0.1), (65, list(range(20, 39)), 0.0, 0.0), (17, [1], 0.3, 0.3)],
                [(511, list(range(1, 39, 2)), 0.2, 0.05), (8, [2, 4], 0.0, 0.5)]]),
]


def targets_of(rng, shapes):
    parts, off = [], [0]
    for rows, labels, p0, p255 in shapes:
        t = rng.choice(labels, rows) if labels else np.zeros(rows, dtype=np.int64)
        u = rng.random(rows)
        t = np.where(u < p0, 0, np.where(u < p0 + p255, IGNORE, t))
        parts.append(t.astype(np.int64))
        off.append(off[-1] + rows)
    return np.concatenate(parts), off


def iou_rows(metrics, num_labels):
    inter = np.full(num_labels, np.nan)
    union = np.full(num_labels, np.nan)
    for label, v in metrics["intersection"].items():
        inter[label] = v
    for label, v in metrics["union"].items():
        union[label] = v
    return inter, union


def main():
    out = {"g12_n": np.array(len(SEQUENCES))}
    criterion = torch.nn.CrossEntropyLoss(ignore_index=IGNORE)                      # trainer_csn.py:406
    for k, (nl, seed, batches) in enumerate(SEQUENCES):
        rng = np.random.default_rng(seed)
        out[f"g12_{k}_cfg"] = np.array([nl, seed, len(batches)])
        losses, scores = ref.AverageMeter(), ref.AverageMeter()
        ious_shape, ious_batch = {}, {}
        for b, shapes in enumerate(batches):
            target_np, off = targets_of(rng, shapes)
            output = torch.from_numpy(g12_logits(seed, b, target_np, nl))
            target = torch.from_numpy(target_np)
            pred = torch.max(output[:, 1:], 1)[1] + 1                               # :466
            num_sample = target.shape[0]
            cross_ent = criterion(output, target.long())                            # :471
            losses.update(float(cross_ent), num_sample)                             # :472
            prec = ref.precision_at_one_partnet(pred, target)
            scores.update(prec, num_sample)                                         # :473
            whole = ref.calculate_iou(ground=target.numpy(), prediction=pred.numpy(), num_labels=nl)     # :474
            ious_batch[b] = whole
            per = []
            for s in range(len(shapes)):
                m = ref.calculate_iou(ground=target[off[s]:off[s + 1]].numpy(), prediction=pred[off[s]:off[s + 1]].numpy(), num_labels=nl)
                ious_shape[len(ious_shape)] = m
                per.append(iou_rows(m, nl))
            pre = f"g12_{k}_{b}_"
            out[pre + "target"] = target_np.astype(np.int16)
            out[pre + "offsets"] = np.array(off, dtype=np.int32)
            out[pre + "loss"] = np.array(float(cross_ent))
            out[pre + "prec"] = np.array(prec)
            out[pre + "inter"] = np.stack([p[0] for p in per])
            out[pre + "union"] = np.stack([p[1] for p in per])
            out[pre + "inter_batch"], out[pre + "union_batch"] = iou_rows(whole, nl)
        for tag, ious in (("final", ious_shape), ("final_batch", ious_batch)):
            out[f"g12_{k}_{tag}"] = np.array([losses.avg, scores.avg, ref.calculate_part_iou(ious=ious, num_labels=nl) * 100,
                                             ref.calculate_shape_iou(ious=ious) * 100])                  # :488-500
    path = os.path.join(HERE, "g12_minkowski_seg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
