"""A fresh numpy / float64 statement of MID-FC/csa_training.py:94-134 — the loss, the accuracy and the Part-IoU counts of one
batch of class-major logits — and the label / logit cases the MID-FC metrics tests share.  Nothing here imports the package.

The reference's sequence, both times: squeeze the trailing axis, transpose to [shape][point][class], flatten to
[point][class], gather the points with label > mask; then cross-entropy + arg-max accuracy (:94-108), or arg-max + a loop over
the classes that counts ``pk & lk`` and ``pk | lk`` (:110-134)."""
import numpy as np


def _gather(logits, labels, mask):
    z = np.asarray(logits, dtype=np.float64)
    if z.ndim == 4:
        z = z[..., 0]
    flat = np.transpose(z, (0, 2, 1)).reshape(-1, z.shape[1])
    lab = np.asarray(labels).reshape(-1)
    keep = np.nonzero(lab > mask)[0]
    return flat[keep], lab[keep]


def loss_accuracy(logits, labels, mask=0):
    """(mean cross-entropy, accuracy) over the gathered points (:94-108); nan for an empty selection, as torch gives."""
    sel, tgt = _gather(logits, labels, mask)
    if len(tgt) == 0:
        return float("nan"), float("nan")
    m = sel.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(sel - m).sum(axis=1))
    nll = lse - sel[np.arange(len(tgt)), tgt]
    return float(nll.mean()), float((sel.argmax(axis=1) == tgt).mean())


def iou_counts(logits, labels, class_num, mask=0):
    """(intsc, union), each (class_num,) — the per-class loop of :124-131 over the gathered points of the whole batch."""
    sel, tgt = _gather(logits, labels, mask)
    pred = sel.argmax(axis=1) if len(tgt) else np.zeros((0,), dtype=np.int64)
    intsc, union = np.zeros(class_num), np.zeros(class_num)
    for k in range(class_num):
        pk, lk = pred == k, tgt == k
        intsc[k] = float((pk & lk).sum())
        union[k] = float((pk | lk).sum())
    return intsc, union


def shape_counts(logits, labels, n_classes, mask=0):
    """(S, n_classes, 3) int64: intersection, ground truth and prediction of the same loop, shape by shape
    (union = gt + pr - inter is asserted against ``pk | lk`` on the way)."""
    z, lab = np.asarray(logits), np.asarray(labels)
    out = np.zeros((z.shape[0], n_classes, 3), dtype=np.int64)
    for s in range(z.shape[0]):
        sel, tgt = _gather(z[s:s + 1], lab[s:s + 1], mask)
        pred = sel.argmax(axis=1) if len(tgt) else np.zeros((0,), dtype=np.int64)
        for k in range(n_classes):
            pk, lk = pred == k, tgt == k
            out[s, k] = ((pk & lk).sum(), lk.sum(), pk.sum())
            assert out[s, k, 1] + out[s, k, 2] - out[s, k, 0] == (pk | lk).sum()
    return out


LABEL_KINDS = ("uniform", "all_masked", "one_class", "some_beyond")
LOGIT_KINDS = ("random", "ties", "neg_inf")


def make_labels(rng, kind, S, N, n_classes, mask):
    if kind == "uniform":
        return rng.integers(0, n_classes, size=(S, N)).astype(np.int64)
    if kind == "all_masked":                                     # every label <= mask: loss nan, every count 0
        return rng.integers(mask - 2, mask + 1, size=(S, N)).astype(np.int64)
    if kind == "one_class":
        return np.full((S, N), n_classes - 1, dtype=np.int64)
    if kind == "some_beyond":                                    # labels n_classes .. n_classes + 2 among valid ones
        return rng.integers(0, n_classes + 3, size=(S, N)).astype(np.int64)
    raise ValueError(kind)


def make_logits(rng, kind, S, N, n_classes):
    if kind == "random":
        return (3.0 * rng.standard_normal(size=(S, n_classes, N))).astype(np.float32)
    if kind == "ties":                                           # three values only: exact ties at the maximum in most points
        return rng.integers(0, 3, size=(S, n_classes, N)).astype(np.float32)
    if kind == "neg_inf":                                        # -inf entries, -inf as a point's first class; the last class stays
        z = rng.standard_normal(size=(S, n_classes, N)).astype(np.float32)     # finite, so that every point has a finite lse
        z[:, :-1][rng.random(size=(S, n_classes - 1, N)) < 0.3] = -np.inf
        z[:, 0, ::2] = -np.inf
        return z
    raise ValueError(kind)
