"""CPU-side checks of the MID-FC test mode (no GPU): the float64 restatement tests/midfc_metrics_ref.py against the host route
of csn_amd.training; the host-side refusals of csn_masked_ce_metrics_fwd_f32; the command line and the summary file of
csn_amd.get_csa_pred; and training.test_layers on CPU tensors.

The loss bound: the host route is torch's fp32 log-softmax of at most 51 logits of magnitude <= ~12 (3 sigma logits, lse <= 16,
ulp 9.5e-7), a handful of roundings per point and a mean — 1e-5 absolute holds it with room and is far below any slip."""
import os

import numpy as np
import pytest
import torch

from tests import midfc_metrics_ref as R

CASES = [(S, C, N) for S, C, N in ((1, 2, 1), (3, 3, 65), (1, 39, 257), (3, 51, 64), (3, 65, 255))]


@pytest.mark.parametrize("S,C,N", CASES)
@pytest.mark.parametrize("labels", R.LABEL_KINDS)
@pytest.mark.parametrize("logits", R.LOGIT_KINDS)
@pytest.mark.parametrize("mask", [0, -1])
def test_restatement_equals_the_host_route(S, C, N, labels, logits, mask):
    from csn_amd import training as T
    rng = np.random.default_rng(S * 1000 + C * 10 + N)
    z, lab = R.make_logits(rng, logits, S, N, C), R.make_labels(rng, labels, S, N, C, mask)
    zt, lt = torch.from_numpy(z).unsqueeze(-1), torch.from_numpy(lab)
    i_t, u_t = T.IoU_per_shape(zt, lt, C, mask)
    i_r, u_r = R.iou_counts(z, lab, C, mask)
    assert i_t.dtype == torch.float32 and i_t.shape == (C,)
    assert np.array_equal(i_t.numpy(), i_r) and np.array_equal(u_t.numpy(), u_r)
    per_shape = R.shape_counts(z, lab, C, mask).sum(axis=0)
    assert np.array_equal(per_shape[:, 0], i_r) and np.array_equal(per_shape[:, 1] + per_shape[:, 2] - per_shape[:, 0], u_r)
    if labels == "some_beyond":                                  # F.cross_entropy refuses a target >= n_classes, as the reference would
        return
    loss_t, accu_t = T.loss_functions_seg(zt, lt, C, mask=mask)
    loss_r, accu_r = R.loss_accuracy(z, lab, mask)
    if labels == "all_masked" or not (lab > mask).any():         # (a single point may draw a masked label)
        assert np.isnan(loss_r) and torch.isnan(loss_t) and not per_shape.any()
        return
    if np.isinf(loss_r):                                         # a labelled class at -inf: both say +inf
        assert loss_t.item() == loss_r
    else:
        assert abs(loss_t.item() - loss_r) < 1e-5
    assert abs(accu_t.item() - accu_r) < 1e-6


# -------------------------------------------------------------------------------------------------------------------------
# the C ABI refuses on the host, before any launch (the fake pointers are never followed)
# -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


def test_metrics_entry_point_refuses_on_the_host(L):
    lib = L.lib()
    S, C, N = 3, 39, 257
    need = lib.csn_masked_ce_metrics_workspace_bytes(S, C, N)
    assert need == lib.csn_masked_ce_workspace_bytes(S, N) == S * 2 * 3 * 8
    assert lib.csn_masked_ce_metrics_workspace_bytes(0, C, N) == 0 and lib.csn_masked_ce_metrics_workspace_bytes(S, 0, N) == 0
    assert lib.csn_masked_ce_metrics_workspace_bytes(S, C, 0) == 0
    names = ["logits", "shape_stride", "ld", "labels", "label_shape_stride", "n_shapes", "n_classes", "n_points", "mask", "lse", "pred",
             "counts", "ws", "ws_bytes", "stats", "stream"]
    valid = dict(logits=4096, shape_stride=C * N, ld=N, labels=8192, label_shape_stride=N, n_shapes=S, n_classes=C, n_points=N, mask=0,
                 lse=None, pred=None, counts=12288, ws=16384, ws_bytes=need, stats=20480, stream=None)

    def call(**change):
        a = dict(valid, **change)
        return lib.csn_masked_ce_metrics_fwd_f32(*[a[k] for k in names])

    for ptr in ("logits", "labels", "counts", "stats", "ws"):
        assert call(**{ptr: None}) == -1, ptr
    for size in ("n_classes", "n_points", "n_shapes"):
        assert call(**{size: 0}) == -1, size
        assert call(**{size: -1}) == -1, size
    assert call(ld=N - 1) == -1                                  # a count beyond its row
    assert call(n_shapes=65536) == -5 and call(n_classes=65536) == -5
    assert call(ws=16388) == -3                                  # fp64 partial sums: 8-byte aligned
    assert call(ws_bytes=need - 1) == -6


# -------------------------------------------------------------------------------------------------------------------------
# python -m csn_amd.get_csa_pred
# -------------------------------------------------------------------------------------------------------------------------
def launcher_argv(logs_dir, name, num_workers=3, batch_size=1, num_classes=15, attention_type="csa", n_heads=8, K=4):
    """run_csa_pred.py:63-78 without the script name."""
    logs_base_dir = os.path.join(logs_dir, "pretrained_models/run_1/")
    knn_graphs_dir = os.path.join(logs_dir, "pretrained_models/knn_graphs", f"n_heads_{n_heads}/{name}")
    return [f"--logs_dir={os.path.join(logs_base_dir, name)}", f"--knn_graphs={knn_graphs_dir}", f"--num_workers={num_workers}",
            f"--batch_size={batch_size}", f"--partname={name}", f"--num_classes={num_classes}", f"--attention_type={attention_type}",
            f"--n_heads={n_heads}", f"--K={K}"]


def test_get_csa_pred_takes_the_launchers_argv(monkeypatch):
    from csn_amd import get_csa_pred as G
    monkeypatch.delenv(G.DATAROOT_ENV, raising=False)
    a = G.build_parser().parse_args(launcher_argv("logs/", "Bed"))
    assert a.logs_dir == "logs/pretrained_models/run_1/Bed" and a.knn_graphs == "logs/pretrained_models/knn_graphs/n_heads_8/Bed"
    assert (a.num_workers, a.batch_size, a.partname, a.num_classes, a.attention_type, a.n_heads, a.K) == (3, 1, "Bed", 15, "csa", 8, 4)
    assert a.testing is False and a.save_pred_dir is None and a.dataroot is None
    monkeypatch.setenv(G.DATAROOT_ENV, "/data/partnet")
    b = G.parse_args(launcher_argv("logs/", "Chair", num_classes=39) + ["--testing", "--save_pred_dir=out"])
    assert b.dataroot == "/data/partnet" and b.testing and b.save_pred_dir == "out" and b.num_classes == 39
    assert G.parse_args(launcher_argv("logs/", "Bed") + ["--dataroot=/elsewhere"]).dataroot == "/elsewhere"


def test_summary_file_has_pandas_bytes(tmp_path):
    from csn_amd import get_csa_pred as G
    p = tmp_path / G.SUMMARY_NAME
    G.write_summary(str(p), "Bed", 45.25)
    assert p.read_bytes() == b",Bed\n0,45.25\n"
    G.write_summary(str(p), "StorageFurniture", 100 * 0.5123456789012345)          # shortest round-trip form, as to_csv writes floats
    assert p.read_bytes() == b",StorageFurniture\n0," + repr(100 * 0.5123456789012345).encode() + b"\n"
    G.write_summary(str(p), "Vase", 0)
    assert p.read_bytes() == b",Vase\n0,0.0\n"


# -------------------------------------------------------------------------------------------------------------------------
# training.test_layers on the host
# -------------------------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """A logit layer alone: (B, C, N, 1) features -> (B, n_cls, N, 1) class-major logits."""

    def __init__(self, channels, n_cls):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(n_cls, channels, generator=g))

    def forward(self, feats, mode, nbrs=None):
        return torch.einsum("kc,bcn->bkn", self.w, feats.squeeze(-1)).contiguous().unsqueeze(-1)


def test_test_layers_on_the_host(tmp_path):
    from torch.utils.data import DataLoader
    from csn_amd import training as T
    from csn_amd.data import SyntheticShapes
    n_cls, N = 6, 64
    ds = SyntheticShapes(5, n_cls, seed=3, n_points=N, channels=8)
    ds.labels[4] = 0                                             # a shape with no labelled point: its batch of one is a NaN batch
    model, dev = _Stub(8, n_cls), torch.device("cpu")
    own = [N, 1, 37, 63, 20]
    names = [(f"shape{i}.npy", own[i]) for i in range(5)]
    res = T.test_layers(model, DataLoader(ds, 2, shuffle=False), n_cls, dev, names=names, save_pred_dir=str(tmp_path / "pred"))
    iou, loss = T.validate_layers(model, DataLoader(ds, 2, shuffle=False), n_cls, dev)
    assert res["part_iou"] == iou and res["loss"] == loss
    assert set(res) == {"part_iou", "loss", "accuracy", "shape_iou", "shapes"} and res["shapes"] == 4

    with torch.no_grad():
        z = model(torch.from_numpy(ds.feats), "test").squeeze(-1).numpy()
    lab = ds.labels
    pred = z.argmax(axis=1)
    sel = lab > 0
    assert abs(res["accuracy"] - (pred[sel] == lab[sel]).mean()) < 1e-12
    counts = R.shape_counts(z, lab, n_cls)
    shape_ious = []
    for s in range(4):
        inter, union = counts[s, 1:, 0], counts[s, 1:, 1] + counts[s, 1:, 2] - counts[s, 1:, 0]
        shape_ious.append(np.mean(inter[union > 0] / union[union > 0]))
    assert abs(res["shape_iou"] - np.mean(shape_ious)) < 1e-12
    for i in range(5):
        saved = np.load(tmp_path / "pred" / f"shape{i}.npy")
        assert saved.dtype == np.int64 and saved.shape == (own[i],)
        assert np.array_equal(saved, pred[i, :own[i]])
    assert sorted(os.listdir(tmp_path / "pred")) == [f"shape{i}.npy" for i in range(5)]

    first = T.test_layers(model, DataLoader(ds, 2, shuffle=False), n_cls, dev, max_batches=1)
    assert first["part_iou"] == T.validate_layers(model, DataLoader(ds, 2, shuffle=False), n_cls, dev, max_batches=1)[0]
