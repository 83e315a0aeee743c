"""GPU checks of the MID-FC metrics pass (include/csn_hip.h section 10, csn_masked_ce_metrics_fwd_f32) and of what is built on it
(csn_amd.functional.masked_ce_metrics, training.IoU_per_shape / validate_layers on the device).

Everything is compared EXACTLY: stats and lse bit for bit with csn_masked_ce_fwd_f32 on the same buffers, pred with
torch.argmax, counts with the float64 restatement tests/midfc_metrics_ref.py (integers), two calls with each other.  The shapes
are the smallest that cross each boundary: a wave (64), a work-group (256), the LDS histogram's class cap (64 classes)."""
import numpy as np
import pytest
import torch

from tests import midfc_metrics_ref as R

pytestmark = pytest.mark.gpu

CANARY_I = -7070707
GUARD = 16
HIST_CAP = 64                                                    # CE_HIST_CLASSES of csn_amd/csrc/loss.hip


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(shape, dtype, fill):
    """A device tensor of ``shape`` inside a flat allocation with GUARD canary elements on either side."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_intact(flat, fill):
    return bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all())


def _place(z, lab, padded):
    """The logits and labels on the device: natural, or — padded — with ld > N, a shape stride with slack, a base 4 bytes off
    16-byte alignment, and label rows with slack; the padding holds nan (logits) / a huge label, so a read of it shows."""
    S, C, N = z.shape
    if not padded:
        return torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda(), (C * N, N, N), None, None
    ld, stride, lstride = N + 3, C * (N + 3) + 5, N + 2
    zbuf = torch.full((1 + S * stride + 7,), float("nan"), device="cuda", dtype=torch.float32)
    zv = zbuf[1:1 + S * stride].view(S, stride)[:, :C * ld].view(S, C, ld)[:, :, :N]
    zv.copy_(torch.from_numpy(z))
    lbuf = torch.full((S * lstride,), 2 ** 40, device="cuda", dtype=torch.int64)
    lv = lbuf.view(S, lstride)[:, :N]
    lv.copy_(torch.from_numpy(lab))
    assert zv.data_ptr() % 16 == 4
    return zv, lv, (stride, ld, lstride), zbuf, lbuf           # (the strides by name: torch renumbers those of one-element axes)


def _parent(L, zv, lv, strides, mask):
    """csn_masked_ce_fwd_f32 on the same buffers: (stats, lse)."""
    lib = L.lib()
    S, C, N = zv.shape
    lse = torch.empty((S, N), device="cuda", dtype=torch.float32)
    stats = torch.empty((3,), device="cuda", dtype=torch.float32)
    wsb = int(lib.csn_masked_ce_workspace_bytes(S, N))
    ws = torch.empty((wsb // 8,), device="cuda", dtype=torch.float64)
    L.check(lib.csn_masked_ce_fwd_f32(zv.data_ptr(), strides[0], strides[1], lv.data_ptr(), strides[2], S, C, N, mask, lse.data_ptr(),
                                      ws.data_ptr(), wsb, stats.data_ptr(), None), "csn_masked_ce_fwd_f32")
    return stats, lse


def _metrics(L, zv, lv, strides, mask, want_lse=True, want_pred=True):
    """csn_masked_ce_metrics_fwd_f32 with canaries around lse, pred and counts; counts start as garbage (the call zeroes them)."""
    lib = L.lib()
    S, C, N = zv.shape
    lse_flat, lse = _guarded((S, N), torch.float32, -77.25)
    pred_flat, pred = _guarded((S, N), torch.int32, CANARY_I)
    cnt_flat, counts = _guarded((S, C, 3), torch.int32, CANARY_I)
    stats = torch.empty((3,), device="cuda", dtype=torch.float32)
    wsb = int(lib.csn_masked_ce_metrics_workspace_bytes(S, C, N))
    ws = torch.empty((wsb // 8,), device="cuda", dtype=torch.float64)
    L.check(lib.csn_masked_ce_metrics_fwd_f32(zv.data_ptr(), strides[0], strides[1], lv.data_ptr(), strides[2], S, C, N, mask,
                                              lse.data_ptr() if want_lse else None, pred.data_ptr() if want_pred else None,
                                              counts.data_ptr(), ws.data_ptr(), wsb, stats.data_ptr(), None),
            "csn_masked_ce_metrics_fwd_f32")
    torch.cuda.synchronize()
    assert _guards_intact(lse_flat, -77.25) and _guards_intact(pred_flat, CANARY_I) and _guards_intact(cnt_flat, CANARY_I)
    if not want_lse:
        assert bool((lse == -77.25).all())
    if not want_pred:
        assert bool((pred == CANARY_I).all())
    return stats, lse, pred, counts


def _check(L, z, lab, mask, padded, nulls=False):
    S, C, N = z.shape
    zv, lv, strides, zbuf, lbuf = _place(z, lab, padded)
    z_before = None if zbuf is None else _bits(zbuf).clone()
    stats0, lse0 = _parent(L, zv, lv, strides, mask)
    stats, lse, pred, counts = _metrics(L, zv, lv, strides, mask)
    assert torch.equal(_bits(stats), _bits(stats0))
    assert torch.equal(_bits(lse), _bits(lse0))
    assert torch.equal(pred.long(), torch.argmax(zv, dim=1))
    want = R.shape_counts(z, lab, C, mask)
    assert np.array_equal(counts.cpu().numpy(), want)
    again = _metrics(L, zv, lv, strides, mask)
    for a, b in zip((stats, lse, pred, counts), again):
        assert torch.equal(_bits(a), _bits(b))
    if nulls:                                                    # pred = NULL and lse = NULL are skipped, the rest is unchanged
        for want_lse, want_pred in ((False, True), (True, False), (False, False)):
            s2, l2, p2, c2 = _metrics(L, zv, lv, strides, mask, want_lse, want_pred)
            assert torch.equal(_bits(s2), _bits(stats)) and torch.equal(c2, counts)
            assert not want_lse or torch.equal(_bits(l2), _bits(lse))
            assert not want_pred or torch.equal(p2, pred)
    if zbuf is not None:                                         # the inputs and their padding are read-only
        assert torch.equal(_bits(zbuf), z_before)
        assert int((lbuf == 2 ** 40).sum()) == S * 2
    return want


@pytest.mark.parametrize("C", [2, 3, 39, 51, HIST_CAP, HIST_CAP + 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_every_point_and_class_edge(L, N, C):
    """Wave and work-group edges x class counts on either side of the histogram's cap, S = 1 and 3, natural and padded."""
    rng = np.random.default_rng(N * 100 + C)
    for S in (1, 3):
        z = R.make_logits(rng, "random", S, N, C)
        lab = R.make_labels(rng, "uniform", S, N, C, 0)
        for padded in (False, True):
            _check(L, z, lab, 0, padded, nulls=(S == 3 and padded))


@pytest.mark.parametrize("C", [39, HIST_CAP + 1])
@pytest.mark.parametrize("mask", [0, -1])
@pytest.mark.parametrize("logits", R.LOGIT_KINDS)
@pytest.mark.parametrize("labels", R.LABEL_KINDS)
def test_every_label_and_logit_case(L, labels, logits, mask, C):
    S, N = 3, 257
    rng = np.random.default_rng(len(labels) * 1000 + len(logits) * 10 + mask + C)
    z, lab = R.make_logits(rng, logits, S, N, C), R.make_labels(rng, labels, S, N, C, mask)
    want = _check(L, z, lab, mask, padded=True)
    if labels == "all_masked":
        assert not want.any()
        zv, lv, strides, _, _ = _place(z, lab, False)
        stats = _metrics(L, zv, lv, strides, mask)[0].cpu()
        assert torch.isnan(stats[0]) and torch.isnan(stats[1]) and stats[2] == 0
    if labels == "some_beyond":                                  # they count a prediction and no ground truth
        sel = lab > mask
        assert want[:, :, 2].sum() == sel.sum() and want[:, :, 1].sum() == (sel & (lab < C)).sum() < sel.sum()
    if logits == "ties":                                         # the ties are there: most points hold their maximum more than once
        assert ((z == z.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.5


def test_a_point_of_nothing_but_minus_infinity(L):
    """Its lse is -inf and its loss nan, as in the parent's pass; its prediction is class 0, as torch.argmax says."""
    rng = np.random.default_rng(9)
    z, lab = R.make_logits(rng, "neg_inf", 3, 65, 5), R.make_labels(rng, "uniform", 3, 65, 5, 0)
    z[1, :, 64] = -np.inf
    _check(L, z, lab, 0, padded=False)


# -------------------------------------------------------------------------------------------------------------------------
# through Python
# -------------------------------------------------------------------------------------------------------------------------
def test_iou_per_shape_on_the_device_equals_its_host_route():
    from csn_amd import training as T
    rng = np.random.default_rng(21)
    for S, C, N, kind, mask in ((3, 39, 1000, "uniform", 0), (2, 6, 257, "some_beyond", 0), (1, HIST_CAP + 1, 300, "uniform", -1),
                                (2, 4, 64, "all_masked", 0)):
        z = torch.from_numpy(R.make_logits(rng, "ties" if C == 6 else "random", S, N, C)).unsqueeze(-1)
        lab = torch.from_numpy(R.make_labels(rng, kind, S, N, C, mask))
        for class_num in (C, C - 1):
            i_h, u_h = T.IoU_per_shape(z, lab, class_num, mask)
            i_d, u_d = T.IoU_per_shape(z.cuda(), lab.cuda(), class_num, mask)
            assert i_d.is_cuda and i_d.dtype == i_h.dtype and i_d.shape == i_h.shape
            assert torch.equal(i_d.cpu(), i_h) and torch.equal(u_d.cpu(), u_h)
            i_t, u_t = T._iou_per_shape_torch(z.cuda(), lab.cuda(), class_num, mask)
            assert torch.equal(i_d, i_t) and torch.equal(u_d, u_t)


class _Stub(torch.nn.Module):
    """A logit layer alone: (B, C, N, 1) features -> (B, n_cls, N, 1) class-major logits."""

    def __init__(self, channels, n_cls):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(n_cls, channels, generator=g))

    def forward(self, feats, mode, nbrs=None):
        return torch.einsum("kc,bcn->bkn", self.w, feats.squeeze(-1)).contiguous().unsqueeze(-1)


def test_validate_and_test_layers_equal_the_torch_composition(tmp_path):
    """validate_layers on the device (one fused call per batch) against the parent's composition — masked_cross_entropy + the
    torch IoU statements — accumulated by the same rule; test_layers' Part IoU, loss and files against them."""
    from torch.utils.data import DataLoader
    from csn_amd import training as T
    from csn_amd.functional import masked_cross_entropy
    from csn_amd.data import SyntheticShapes
    n_cls, N = 6, 300
    ds = SyntheticShapes(5, n_cls, seed=3, n_points=N, channels=8)
    ds.labels[4] = 0                                             # the last batch (one shape) is a NaN batch
    dev = torch.device("cuda")
    model = _Stub(8, n_cls).to(dev)
    loader = lambda: DataLoader(ds, 2, shuffle=False)
    iou, loss = T.validate_layers(model, loader(), n_cls, dev)

    intsc = torch.zeros(n_cls, device=dev, dtype=torch.float64)
    union = torch.zeros(n_cls, device=dev, dtype=torch.float64)
    total, n, preds = torch.zeros((), device=dev, dtype=torch.float64), 0, []
    with torch.no_grad():
        for feats, label in loader():
            out = model(feats.squeeze(1).to(dev), "test")
            l_b = masked_cross_entropy(out, label.to(dev), 0)[0]
            i_b, u_b = T._iou_per_shape_torch(out, label.to(dev), n_cls)
            ok = (~torch.isnan(l_b)).double()
            total += torch.where(torch.isnan(l_b), torch.zeros_like(l_b), l_b).double()
            intsc += i_b.double() * ok
            union += u_b.double() * ok
            preds.append(out.squeeze(-1).argmax(dim=1).cpu())
            n += 1
    assert n == 3 and iou == T.mean_iou(intsc, union) and loss == float(total.item()) / n

    own = [N, 1, 255, 256, 20]
    res = T.test_layers(model, loader(), n_cls, dev, names=[(f"s{i}.npy", own[i]) for i in range(5)], save_pred_dir=str(tmp_path))
    assert res["part_iou"] == iou and res["loss"] == loss and res["shapes"] == 4
    pred = torch.cat(preds).numpy()
    for i in range(5):
        saved = np.load(tmp_path / f"s{i}.npy")
        assert saved.dtype == np.int64 and np.array_equal(saved, pred[i, :own[i]])
    sel = ds.labels[:4] > 0                                      # (integers: the quotient is the same double)
    assert res["accuracy"] == float((pred[:4][sel] == ds.labels[:4][sel]).sum()) / float(sel.sum())


def test_get_csa_pred_cli_end_to_end(tmp_path, monkeypatch):
    """``python -m csn_amd.get_csa_pred`` through its main() with EXACTLY the argv run_csa_pred.py:67-78 builds (+ --save_pred_dir):
    feature files in the O-CNN layout, a saved CSA checkpoint and a test graph in, out come the reference's log lines, the
    summary file with validate_layers' Part IoU on the same loader, and every shape's own points as int64 predictions."""
    from torch.utils.data import DataLoader
    from csn_amd import get_csa_pred as G
    from csn_amd import training as T
    from csn_amd.csa_models import get_model
    from csn_amd.data import CSADatasetK
    from tests.test_cpu_midfc_metrics import launcher_argv
    rng = np.random.default_rng(9)
    n_cls, part, K = 4, "Bottle", 1
    root = tmp_path / "data"
    sizes = {"train": [10000, 7000, 10000], "test": [10000, 6000]}                       # short shapes are wrap-around padded
    for split, ns in sizes.items():
        d = root / f"{split}_data_features" / part
        (d / "fc_1").mkdir(parents=True)
        (d / "point_labels").mkdir()
        for i, n in enumerate(ns):
            np.save(d / "fc_1" / f"shape_{i:02d}.npy", (rng.standard_normal((1, 256, n, 1)) + 0.3 * i).astype(np.float32))
            np.save(d / "point_labels" / f"shape_{i:02d}.npy", rng.integers(0, n_cls, size=n))
    torch.manual_seed(1)
    model = get_model("csa", n_cls, 1, K).cuda().eval()
    logs = tmp_path / "logs"
    argv = launcher_argv(str(logs), part, num_workers=0, num_classes=n_cls, n_heads=1, K=K)
    a = G.build_parser().parse_args(argv)
    (tmp_path / a.logs_dir).mkdir(parents=True, exist_ok=True)
    torch.save(model.state_dict(), str(tmp_path / a.logs_dir / "trained_layers.pth"))
    (tmp_path / a.knn_graphs).mkdir(parents=True, exist_ok=True)
    graph = np.array([[2, 0, 1], [1, 2, 0]], dtype=np.int64)
    np.save(str(tmp_path / a.knn_graphs / "test.npy"), graph)
    monkeypatch.setenv(G.DATAROOT_ENV, str(root))
    res = G.main(argv + [f"--save_pred_dir={tmp_path / 'pred'}"])

    test_root, train_root = str(root / "test_data_features" / part), str(root / "train_data_features" / part)
    ds = CSADatasetK(test_root, train_root, graph, K)
    iou, loss = T.validate_layers(model, DataLoader(ds, 1, shuffle=False), n_cls, torch.device("cuda"))
    assert res["part_iou"] == iou and res["loss"] == loss and res["shapes"] == 2
    assert (tmp_path / a.logs_dir / G.SUMMARY_NAME).read_bytes() == f",{part}\n0,{iou * 100!r}\n".encode()
    lines = (tmp_path / a.logs_dir / "logs.txt").read_text().splitlines()
    assert lines[0] == f"model wts loaded from {tmp_path / a.logs_dir / 'trained_layers.pth'}!" and lines[1] == "---- Validation ----"
    assert lines[2] == f"Final shape_IoU: {iou * 100}" and lines[-1] == f"test IoU saved to {tmp_path / a.logs_dir / G.SUMMARY_NAME}"
    for name in ds.own.files:
        n_own = len(np.load(root / "test_data_features" / part / "point_labels" / name))
        saved = np.load(tmp_path / "pred" / name)
        assert saved.dtype == np.int64 and saved.shape == (n_own,) and saved.min() >= 0 and saved.max() < n_cls


def test_masked_ce_metrics_is_masked_cross_entropy_with_more_outputs():
    from csn_amd.functional import masked_ce_metrics, masked_cross_entropy
    from csn_amd import _lib
    rng = np.random.default_rng(33)
    S, C, N = 3, 39, 257
    z = torch.from_numpy(R.make_logits(rng, "random", S, N, C)).cuda()
    lab = torch.from_numpy(R.make_labels(rng, "uniform", S, N, C, 0)).cuda()
    a = z.clone().unsqueeze(-1).requires_grad_(True)
    b = z.clone().unsqueeze(-1).requires_grad_(True)
    loss_a, accu_a, cnt_a = masked_cross_entropy(a, lab, 0)
    loss_b, accu_b, cnt_b, pred, counts = masked_ce_metrics(b, lab, 0)
    assert torch.equal(loss_a, loss_b) and torch.equal(accu_a, accu_b) and torch.equal(cnt_a, cnt_b)
    assert pred.dtype == torch.int32 and torch.equal(pred.long(), z.argmax(dim=1))
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), R.shape_counts(z.cpu().numpy(), lab.cpu().numpy(), C))
    assert not pred.requires_grad and not counts.requires_grad and loss_b.requires_grad
    (loss_a * 1.5).backward()
    (loss_b * 1.5).backward()
    assert a.grad.shape == b.grad.shape and torch.equal(a.grad, b.grad) and bool(b.grad.abs().sum() > 0)
    assert masked_ce_metrics(z, lab, 0, want_pred=False)[3] is None
    # it refuses what masked_cross_entropy refuses
    for bad_z, bad_l in ((z.half(), lab), (z, lab.int()), (z.cpu(), lab.cpu()), (z, lab[:, :-1]), (z.permute(0, 2, 1), lab)):
        with pytest.raises(_lib.CsnError):
            masked_ce_metrics(bad_z, bad_l, 0)
        with pytest.raises(_lib.CsnError):
            masked_cross_entropy(bad_z, bad_l, 0)
