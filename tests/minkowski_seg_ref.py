"""float64 / numpy restatement of what lies between the MinkowskiNet head's logits and its reported numbers
(MinkowskiNet/lib/trainer_csn.py:400-500, lib/utils.py:64-176), written independently of csn_amd: the yardstick of
include/csn_hip.h section (12) and of csn_amd/minkowski_training.py.  tests/test_cpu_minkowski_seg.py pins it to goldens that
the reference's own functions produced (tests/golden/g12_minkowski_seg.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_minkowski_seg.npz")


def g12_logits(seed, batch, target, num_labels):
    """The fp32 logits of batch ``batch`` of a G12 sequence: a seeded stream (numpy's default_rng is version-stable), the target
    class raised on ~60 % of the rows so that the precision is neither 0 nor 100, and an exact TIE between two classes that
    both beat every other on every 17th row (classes 2 and 4; 1 and 3 with four labels)."""
    target = np.asarray(target)
    rng = np.random.default_rng([seed, batch])
    z = rng.standard_normal((target.shape[0], num_labels)).astype(np.float32)
    lift = (rng.random(target.shape[0]) < 0.6) & (target >= 1) & (target < num_labels)
    rows = np.nonzero(lift)[0]
    z[rows, target[rows]] += np.float32(2.5)
    a, b = (2, 4) if num_labels > 4 else (1, 3)
    tie = np.arange(3, target.shape[0], 17)
    top = z[tie].max(axis=1) + np.float32(1.0)
    z[tie, a] = top
    z[tie, b] = top
    return z


def seg_ref(logits, labels, offsets, n_classes, ignore_label=255, grad_out=1.0):
    """Section (12) in float64.  Returns a dict: lse (N,), pred (N,), loss, n_counted, n_correct, n_bad, counts (S, n_classes, 3)
    int64 (intersection, ground truth, prediction), dlogits (N, n_classes)."""
    z = np.asarray(logits)[:, :n_classes].astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    N = z.shape[0]
    with np.errstate(all="ignore"):
        m = z.max(axis=1, keepdims=True)
        e = np.where(z == m, 1.0, np.exp(z - m))                 # (-inf - -inf: a row of -inf only)
        lse = (m + np.log(e.sum(axis=1, keepdims=True)))[:, 0]
    pred = 1 + np.argmax(z[:, 1:], axis=1)                       # the first maximum, as torch.max(output[:, 1:], 1)[1] + 1
    valid = (lab >= 0) & (lab < n_classes)
    ignored = lab == ignore_label
    counted = valid & ~ignored
    bad = ~valid & ~ignored
    rows = np.nonzero(counted)[0]
    per_row = lse[rows] - z[rows, lab[rows]]
    n_counted = int(counted.sum())
    loss = float(per_row.sum() / n_counted) if n_counted else float("nan")
    n_correct = int((counted & ((pred == lab) | (lab == 0))).sum())
    pz = np.where(lab == 0, 0, pred)                             # calculate_iou: prediction[ground == 0] = 0
    S = len(offsets) - 1
    seg = np.searchsorted(np.asarray(offsets, dtype=np.int64), np.arange(N), side="right") - 1
    counts = np.zeros((S, n_classes, 3), dtype=np.int64)
    g_rows = np.nonzero(valid)[0]                                # (a valid row is never bad)
    p_rows = np.nonzero(~bad)[0]
    i_rows = np.nonzero(valid & (pz == lab))[0]
    np.add.at(counts, (seg[i_rows], lab[i_rows], 0), 1)
    np.add.at(counts, (seg[g_rows], lab[g_rows], 1), 1)
    np.add.at(counts, (seg[p_rows], pz[p_rows], 2), 1)
    d = np.zeros((N, n_classes), dtype=np.float64)
    if n_counted:
        with np.errstate(all="ignore"):
            prob = np.where(np.isneginf(z), 0.0, np.exp(z - lse[:, None]))
        onehot = np.zeros_like(prob)
        onehot[rows, lab[rows]] = 1.0
        d[rows] = (prob[rows] - onehot[rows]) * (float(grad_out) / n_counted)
    return {"lse": lse, "pred": pred.astype(np.int64), "loss": loss, "n_counted": n_counted, "n_correct": n_correct,
            "n_bad": int(bad.sum()), "counts": counts, "dlogits": d}


def precision_ref(r):
    """precision_at_one_partnet (utils.py:64-75) from the restatement's sums, 0..100."""
    return 100.0 * r["n_correct"] / r["n_counted"] if r["n_counted"] else float("nan")


def iou_arrays(counts_s):
    """One segment's (n_classes, 3) counts -> calculate_iou's intersection and union per label as float64 arrays of n_classes
    entries, nan where the reference's dicts have no key (label 0, and labels whose union is 0)."""
    inter = counts_s[:, 0].astype(np.float64)
    union = (counts_s[:, 1] + counts_s[:, 2] - counts_s[:, 0]).astype(np.float64)
    absent = union <= 0
    absent[0] = True
    return np.where(absent, np.nan, inter), np.where(absent, np.nan, union)


class MeterRef:
    """losses / scores / ious of Trainer.test (trainer_csn.py:407, 472-475) and its last four lines (:488-500), in Python floats."""

    def __init__(self, num_labels):
        self.n = num_labels
        self.loss_sum = self.score_sum = 0.0
        self.rows = 0
        self.ious = []                                           # per segment: (intersection, union) arrays

    def update(self, r, n_rows):
        self.loss_sum += r["loss"] * n_rows
        self.score_sum += precision_ref(r) * n_rows
        self.rows += n_rows
        self.ious += [iou_arrays(c) for c in r["counts"]]

    def result(self):
        inter = np.zeros(self.n)
        union = np.zeros(self.n)
        shape_ious = []
        for i_s, u_s in self.ious:
            keep = ~np.isnan(u_s)
            inter[keep] += i_s[keep]
            union[keep] += u_s[keep]
            if keep.any():
                shape_ious.append(float(np.sum(i_s[keep] / u_s[keep]) / keep.sum()))
        part = sum(inter[i] / union[i] if union[i] > 0 else 0.0 for i in range(1, self.n)) / float(self.n - 1)
        shape = float(np.sum(shape_ious) / len(shape_ious)) if shape_ious else float("nan")
        return self.loss_sum / self.rows, self.score_sum / self.rows, part * 100, shape * 100


def g12_sequences(path=GOLDEN):
    """The sequences of the golden file: [(num_labels, seed, [batch dict])], a batch dict holding target, offsets, the regenerated
    logits and every number the reference gave for it; plus the sequence's final numbers."""
    g = np.load(path)
    out = []
    for k in range(int(g["g12_n"])):
        nl, seed, nb = (int(v) for v in g[f"g12_{k}_cfg"])
        batches = []
        for b in range(nb):
            pre = f"g12_{k}_{b}_"
            target = g[pre + "target"].astype(np.int64)
            batches.append({"target": target, "offsets": g[pre + "offsets"].astype(np.int64).tolist(),
                            "logits": g12_logits(seed, b, target, nl), "loss": float(g[pre + "loss"]), "prec": float(g[pre + "prec"]),
                            "inter": g[pre + "inter"], "union": g[pre + "union"],
                            "inter_batch": g[pre + "inter_batch"], "union_batch": g[pre + "union_batch"]})
        out.append({"num_labels": nl, "seed": seed, "batches": batches, "final": g[f"g12_{k}_final"], "final_batch": g[f"g12_{k}_final_batch"]})
    return out
