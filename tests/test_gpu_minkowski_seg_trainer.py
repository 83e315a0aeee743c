"""``SegTrainer`` and ``test_split`` on the device (csn_amd/minkowski_trainer.py), and test mode of the two command lines in child
processes: a resumed ``HRNetSeg`` run against an uninterrupted one bit for bit, ``validate`` and ``test_split`` against ``evaluate`` by
hand, the files ``train()`` and test mode leave on disk.

The setting of every test is that of tests/test_gpu_minkowski_trainer.py: ellipsoid shells of 150-260 points with unequal counts — 6
training, 3 validation, 3 test —, labels folded to 1..3 (4 classes), ``voxel_size`` 0.05, ``batch_size`` 2, SGD, PolyLR;
``HRNetSeg2S(3, 4)`` and ``HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=1)``.  An ``HRNetSeg`` epoch is ceil(6 / 2) = 3
iterations.  ``_collections`` asserts that the coarsest level keeps at least 3 rows for every single shape even at the smallest
augmentation scale and that some shape's voxel count is no multiple of 32.

Every equality is exact: no kernel on this path uses floating-point atomics and evaluation draws nothing."""
import functools
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import csn_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.05
N_TRAIN, N_VAL, N_TEST, N_CLASSES = 6, 3, 3, 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    csn_amd.build()


@functools.lru_cache(maxsize=None)
def _collections():
    from csn_amd import AugmentSpec, PointCollection
    from csn_amd.train_csn import synthetic_shapes
    pts, labs = synthetic_shapes(N_TRAIN + N_VAL + N_TEST, seed=3)
    labs = [(1 + (l - 1) % (N_CLASSES - 1)).astype(np.int32) for l in labs]          # octants folded onto the labels 1..3
    counts = [p.shape[0] for p in pts]
    assert all(150 <= c <= 260 for c in counts) and len(set(counts[:N_TRAIN])) == N_TRAIN and len(set(counts[-N_TEST:])) == N_TEST
    smallest = AugmentSpec().scale_bound[0]
    for p in pts:                                                                    # level 1 of the 2S pyramid: tensor stride 2
        coarse = np.unique(np.floor(np.floor(p.astype(np.float64) * smallest / VOXEL) / 2), axis=0)
        assert coarse.shape[0] >= 3
    cut = (0, N_TRAIN, N_TRAIN + N_VAL, len(pts))
    train, val, test = (PointCollection(pts[a:b], labs[a:b]) for a, b in zip(cut, cut[1:]))
    voxels = [col.batch([i], voxel_size=VOXEL).field().n_voxels for col in (train, test) for i in range(col.n_shapes)]
    assert any(v % 32 for v in voxels), voxels
    return train, val, test


def _cfg(log_dir, model, **cfg_kw):
    from csn_amd import TrainConfig
    kw = dict(lr=0.05, optimizer="SGD", scheduler="PolyLR", max_iter=100, batch_size=2, voxel_size=VOXEL, stat_freq=1, log_dir=str(log_dir),
              model=model)
    kw.update(cfg_kw)
    return TrainConfig(**kw)


def _trainer(log_dir, model_seed=11, seed=0, **cfg_kw):
    from csn_amd import HRNetSeg2S, SegTrainer
    train, val, _ = _collections()
    torch.manual_seed(model_seed)
    return SegTrainer(HRNetSeg2S(3, N_CLASSES).cuda(), train, val, _cfg(log_dir, "HRNetSeg2S", **cfg_kw), seed=seed)


def _momentum(trainer):
    state = trainer.optimizer.state_dict()["state"]
    return [(i, state[i]["momentum_buffer"]) for i in sorted(state)]


def _differing(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    return [k for k in sa if not torch.equal(sa[k], sb[k])]


def _clone(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def _untouched(model, before):
    now = model.state_dict()
    return list(now) == list(before) and all(torch.equal(v, before[k]) for k, v in now.items())


# ------------------------------------------------------------------------------------------------------
# SegTrainer
# ------------------------------------------------------------------------------------------------------
def test_seg_resume_is_exact(tmp_path):
    """Run A: two epochs in one go.  Run B: one epoch, ``save_checkpoint``, a fresh trainer on a differently initialised model with
    differently seeded generators, ``load_checkpoint``, one more epoch."""
    a = _trainer(tmp_path / "a")
    start = _clone(a.model)
    loss_a = [a.train_epoch(), a.train_epoch()]

    b1 = _trainer(tmp_path / "b")
    loss_b = [b1.train_epoch()]
    path = str(tmp_path / "b" / "mid.pth")
    b1.save_checkpoint(path)
    b2 = _trainer(tmp_path / "b", model_seed=999, seed=5)
    assert not torch.equal(b2.model.final[3].weight, b1.model.final[3].weight)
    b2.load_checkpoint(path)
    loss_b.append(b2.train_epoch())

    assert all(np.isfinite(v) for pair in loss_a for v in pair) and loss_a == loss_b
    sa = a.model.state_dict()
    moved = [k for k in sa if not torch.equal(sa[k], start[k])]
    assert any(k.endswith("running_var") for k in moved) and any(k.endswith("kernel") for k in moved) and "final.3.weight" in moved
    assert _differing(a.model, b2.model) == []
    ma, mb = _momentum(a), _momentum(b2)
    assert len(ma) > 0 and [i for i, _ in ma] == [i for i, _ in mb] and all(torch.equal(x[1], y[1]) for x, y in zip(ma, mb))
    assert a.iters_per_epoch == 3 and a.lr == b2.lr == 0.05 * (1 - 6 / 101) ** 0.9
    assert (a.curr_iter, a.scheduler.last_epoch) == (b2.curr_iter, b2.scheduler.last_epoch) == (7, 6)
    assert (a.epoch, b2.epoch) == (1, 2)                                             # train_epoch leaves it; a file holds epoch + 1
    assert a.sampler.state_dict() == b2.sampler.state_dict() and a.sampler.state_dict()["pos"] == N_TRAIN    # two whole permutations
    assert a.aug_rng.bit_generator.state == b2.aug_rng.bit_generator.state


def test_seg_validate_is_evaluate_on_the_same_fields_and_leaves_the_model_alone():
    from csn_amd import evaluate
    t = _trainer("unused")
    t.train_epoch()
    assert t.model.training
    before = _clone(t.model)
    got = t.validate()
    assert t.model.training and _untouched(t.model, before)

    _, val, _ = _collections()
    batches = []
    for i in range(N_VAL):
        q = val.batch([i], voxel_size=VOXEL)
        batches.append((q.field(), q.labels))

    def forward_fn(field):
        return field.interpolate(t.model(field.sparse())), field.offsets
    t.model.eval()
    want = evaluate(forward_fn, batches, N_CLASSES, 255)
    print("validate", got, "by hand", want)
    assert len(got) == 4 and all(np.isfinite(v) for v in got) and got == want
    assert 0 <= got[1] <= 100 and 0 <= got[2] <= 100 and 0 <= got[3] <= 100
    t.model.eval()
    t.validate()
    assert not t.model.training                                                      # the mode found is the mode left


def test_seg_train_writes_its_files_and_resumes_to_where_an_uninterrupted_run_ends(tmp_path):
    a = _trainer(tmp_path / "a", max_epoch=3)
    a.train()
    b1 = _trainer(tmp_path / "b", max_epoch=2)
    b1.train()
    log_dir = str(tmp_path / "b")
    link = os.path.join(log_dir, "weights.pth")
    assert os.path.islink(link) and os.readlink(link) == "checkpoint_HRNetSeg2S.pth" and os.path.isfile(os.path.join(log_dir, "config.json"))
    state = torch.load(link)
    assert (state["iteration"], state["epoch"], state["arch"]) == (7, 3, "HRNetSeg2S") and "csn_data" not in state
    st = b1.state
    assert st.best_val_loss < float("inf") and st.best_val_loss_iter in (4, 7)       # the first validation always moves the loss
    for postfix, it in (("best_part_iou", st.best_val_part_iou_iter), ("best_shape_iou", st.best_val_shape_iou_iter),
                        ("best_loss", st.best_val_loss_iter), ("best_acc", st.best_val_acc_iter)):
        assert os.path.isfile(b1.checkpoint_path(postfix)) == (it > 0), postfix
        if it > 0:
            assert torch.load(b1.checkpoint_path(postfix))["iteration"] == it
    assert state["best_val_loss_iter"] == 4                                          # the current file precedes the last best values

    b2 = _trainer(tmp_path / "b", model_seed=999, seed=5, max_epoch=3, resume=log_dir)
    b2.train()
    assert (b2.epoch, b2.curr_iter, b2.lr) == (a.epoch, a.curr_iter, a.lr) == (3, 10, 0.05 * (1 - 9 / 101) ** 0.9)
    assert _differing(a.model, b2.model) == []
    fa, fb = torch.load(a.checkpoint_path()), torch.load(b2.checkpoint_path())
    assert (fa["iteration"], fa["epoch"]) == (fb["iteration"], fb["epoch"]) == (10, 4)


# ------------------------------------------------------------------------------------------------------
# test_split
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trained_csn():
    """An ``HRNetSimCSN2S`` after one trained epoch (random graph, K = 1).  Shared: no test may change it."""
    from csn_amd import CSNTrainer, HRNetSimCSN2S
    train, val, _ = _collections()
    torch.manual_seed(11)
    model = HRNetSimCSN2S(3, N_CLASSES, d_model=64, n_head=2, k_neighbors=1).cuda()
    t = CSNTrainer(model, train, val, _cfg("unused", "HRNetSimCSN2S", k_neighbors=1), seed=0)
    t.construct_graphs(recalculate=False)
    t.train_epoch()
    return model


def _rows(model, col, batch_size):
    out = []
    with torch.no_grad():
        for lo in range(0, col.n_shapes, batch_size):
            rows, off = model.backbone_rows(col.batch(list(range(lo, min(lo + batch_size, col.n_shapes))), voxel_size=VOXEL).field().sparse())
            off = off.tolist()
            out += [rows[a:b] for a, b in zip(off, off[1:])]
    return out


def _by_hand(model, test, train, neighbors, batch_size):
    """``evaluate`` on batches built here, in eval mode; the mode found is restored."""
    from csn_amd import HRNetSeg, evaluate
    batches = []
    for lo in range(0, test.n_shapes, batch_size):
        idx = list(range(lo, min(lo + batch_size, test.n_shapes)))
        q = test.batch(idx, voxel_size=VOXEL)
        keys = train.neighbor_batches([neighbors[i] for i in idx], 1, None, VOXEL) if neighbors else []
        batches.append(((q.field(), [k.field() for k in keys]), q.labels))

    def forward_fn(batch):
        field, keys = batch
        if isinstance(model, HRNetSeg):
            return field.interpolate(model(field.sparse())), field.offsets
        return field.interpolate(model(field.sparse(), [k.sparse() for k in keys] or None)), field.offsets
    was_training = model.training
    model.eval()
    try:
        return evaluate(forward_fn, batches, N_CLASSES, 255)
    finally:
        model.train(was_training)


def _file_text(result):
    return "Shape IoU: " + str(np.round(result[3], 2)) + "\nPart IoU: " + str(np.round(result[2], 2))


def test_test_split_csn_ranks_the_test_split_against_the_training_split(tmp_path):
    from csn_amd import minkowski_trainer
    from csn_amd.minkowski_csn import construct_shape_graph
    model = _trained_csn()
    train, _, test = _collections()
    model.train()
    before = _clone(model)
    out = tmp_path / "results"
    with mock.patch.object(minkowski_trainer, "construct_shape_graph", wraps=minkowski_trainer.construct_shape_graph) as graph:
        got = csn_amd.test_split(model, test, train_collection=train, k_neighbors=1, voxel_size=VOXEL, save_pred_dir=str(out))
    assert model.training and _untouched(model, before)
    assert graph.call_count == 1 and graph.call_args.args[0] is model.head and graph.call_args.args[3] == 1

    model.eval()
    neighbors = construct_shape_graph(model.head, _rows(model, test, 1), _rows(model, train, 1), 1)
    model.train()
    assert [q for q, _ in neighbors] == list(range(N_TEST)) and all(len(nb) == 1 and nb[0] in range(N_TRAIN) for _, nb in neighbors)
    want = _by_hand(model, test, train, neighbors, 1)
    print("test_split", got, "by hand", want, "neighbours", neighbors)
    assert len(got) == 4 and all(np.isfinite(v) for v in got) and got == want
    assert 0 <= got[1] <= 100 and 0 <= got[2] <= 100 and 0 <= got[3] <= 100
    assert os.listdir(str(out)) == ["results_log.txt"] and (out / "results_log.txt").read_bytes() == _file_text(got).encode()

    # again, into another empty directory and from eval mode: the same tuple, the same file; the first directory is now refused
    model.eval()
    again = csn_amd.test_split(model, test, train_collection=train, k_neighbors=1, voxel_size=VOXEL, save_pred_dir=str(tmp_path / "again"))
    assert not model.training and again == got and _untouched(model, before)
    assert (tmp_path / "again" / "results_log.txt").read_bytes() == (out / "results_log.txt").read_bytes()
    with pytest.raises(ValueError, match="not empty"):
        csn_amd.test_split(model, test, train_collection=train, k_neighbors=1, voxel_size=VOXEL, save_pred_dir=str(out))
    model.train()


@pytest.mark.parametrize("family", ["csn", "seg"])
def test_test_split_in_batches_of_two_with_a_short_last_batch(family):
    from csn_amd import HRNetSeg2S, minkowski_training
    from csn_amd.minkowski_csn import construct_shape_graph
    train, _, test = _collections()
    if family == "csn":
        model = _trained_csn()
        model.eval()
        neighbors = construct_shape_graph(model.head, _rows(model, test, 2), _rows(model, train, 2), 1)
        model.train()
    else:
        torch.manual_seed(4)
        model, neighbors = HRNetSeg2S(3, N_CLASSES).cuda(), None
    before = _clone(model)
    seen = []
    seg_loss = minkowski_training.seg_loss

    def counted(logits, target, offsets=None, ignore_label=255):
        seen.append((int(logits.shape[0]), len(offsets) - 1))
        return seg_loss(logits, target, offsets, ignore_label)
    with mock.patch.object(minkowski_training, "seg_loss", side_effect=counted):
        got = csn_amd.test_split(model, test, train_collection=train, k_neighbors=1, voxel_size=VOXEL, test_batch_size=2)
    assert [s for _, s in seen] == [2, 1] and sum(n for n, _ in seen) == test.n_points          # per shape, every point once
    want = _by_hand(model, test, train, neighbors, 2)
    print(family, "test_split", got, "by hand", want)
    assert all(np.isfinite(v) for v in got) and got == want
    assert model.training and _untouched(model, before)


@pytest.mark.parametrize("family", ["seg", "csn_k0"])
def test_test_split_without_neighbours_needs_no_training_split(family, tmp_path):
    from csn_amd import HRNetSeg2S, HRNetSimCSN2S
    _, _, test = _collections()
    torch.manual_seed(4)
    if family == "seg":
        model = HRNetSeg2S(3, N_CLASSES).cuda()
        got = csn_amd.test_split(model, test, k_neighbors=1, voxel_size=VOXEL, save_pred_dir=str(tmp_path))    # k_neighbors is ignored
    else:
        model = HRNetSimCSN2S(3, N_CLASSES, d_model=64, n_head=2, k_neighbors=0).cuda()
        got = csn_amd.test_split(model, test, k_neighbors=0, voxel_size=VOXEL, save_pred_dir=str(tmp_path))
    want = _by_hand(model, test, None, None, 1)
    print(family, "test_split", got, "by hand", want)
    assert all(np.isfinite(v) for v in got) and got == want and model.training
    assert (tmp_path / "results_log.txt").read_bytes() == _file_text(got).encode()


# ------------------------------------------------------------------------------------------------------
# the command lines, in child processes
# ------------------------------------------------------------------------------------------------------
TEST_LINES = ("Test split Part IOU: ", "Test split Shape IOU: ", "Test split Loss: ", "Test Score: ")


def _child(module, *args):
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", module, "--synthetic", "6", "--batch_size", "2", "--scheduler", "PolyLR", *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)


@pytest.mark.parametrize("module,model_args,suffix", [
    ("csn_amd.train_seg", ("--model", "HRNetSeg2S"), " at iter 4"),
    ("csn_amd.train_csn", ("--model", "HRNetSimCSN2S", "--d_model", "64", "--n_head", "2", "--k_neighbors", "1"), " at iter 4 (K=1)")])
def test_command_line_trains_then_tests_in_child_processes(tmp_path, module, model_args, suffix):
    from csn_amd.collect_partnet_results import collect_results
    log_dir = tmp_path / "Synthetic-k1-run"
    res = _child(module, "--max_epoch", "1", "--log_dir", str(log_dir), *model_args)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    weights = log_dir / "weights.pth"
    assert torch.load(str(weights))["iteration"] == 4                                # 3 iterations ran; the next is 4

    # --save_pred_dir defaults to <log_dir>/results
    res = _child(module, "--is_train", "False", "--weights", str(weights), "--log_dir", str(log_dir / "evaluation"), *model_args)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [[l for l in res.stdout.splitlines() if head in l] for head in TEST_LINES]
    assert all(len(l) == 1 and l[0].endswith(suffix) for l in lines), res.stdout[-2000:]
    text = (log_dir / "evaluation" / "results" / "results_log.txt").read_text()
    shape_line, part_line = text.split("\n")
    assert shape_line.startswith("Shape IoU: ") and part_line.startswith("Part IoU: ")
    shape_iou, part_iou = float(shape_line.split()[-1]), float(part_line.split()[-1])
    assert 0 <= shape_iou <= 100 and 0 <= part_iou <= 100
    logged = float(lines[0][0].split("Test split Part IOU: ")[1].split()[0])
    assert abs(logged - part_iou) <= 0.00551                                         # {:.3f} in the log (0.0005) + np.round(., 2) in the file (0.005)
    assert collect_results(str(tmp_path)) == collect_results(str(tmp_path), "1") == ([part_iou], [shape_iou])
