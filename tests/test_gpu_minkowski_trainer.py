"""``CSNTrainer`` on the device (csn_amd/minkowski_trainer.py): a resumed run against an uninterrupted one bit for bit, gradient
accumulation, one patience-driven rebuild inside ``train()``, the command line in a child process, and ``validate`` against
``evaluate`` by hand.

The setting of every test: ``HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=1)`` (dropout 0.1, so the dropout seeds matter),
6 training and 3 validation ellipsoid shells of 150-260 points with unequal counts, ``voxel_size`` 0.05, ``batch_size`` 2,
``iter_size`` 2, SGD, PolyLR: an epoch is ceil(6 / 2 / 2) = 2 iterations and draws 8 shapes, so it ends in the middle of the
sampler's second permutation.  At this voxel size nearly every point has a voxel of its own; ``_collections`` asserts that the
coarsest level keeps at least 3 rows for every single shape even at the smallest augmentation scale (a two-row training BatchNorm is
ill-conditioned by construction) and that some shape's voxel count is no multiple of 32."""
import functools
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.05
N_TRAIN, N_VAL, N_CLASSES = 6, 3, 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    import csn_amd
    csn_amd.build()


@functools.lru_cache(maxsize=None)
def _collections():
    from csn_amd import AugmentSpec, PointCollection
    from csn_amd.train_csn import synthetic_shapes
    pts, labs = synthetic_shapes(N_TRAIN + N_VAL, seed=3)
    labs = [(1 + (l - 1) % (N_CLASSES - 1)).astype(np.int32) for l in labs]          # octants folded onto the labels 1..3
    counts = [p.shape[0] for p in pts]
    assert all(150 <= c <= 260 for c in counts) and len(set(counts[:N_TRAIN])) == N_TRAIN
    smallest = AugmentSpec().scale_bound[0]
    for p in pts:                                                                    # level 1 of the 2S pyramid: tensor stride 2
        coarse = np.unique(np.floor(np.floor(p.astype(np.float64) * smallest / VOXEL) / 2), axis=0)
        assert coarse.shape[0] >= 3
    train, val = PointCollection(pts[:N_TRAIN], labs[:N_TRAIN]), PointCollection(pts[N_TRAIN:], labs[N_TRAIN:])
    voxels = [train.batch([i], voxel_size=VOXEL).field().n_voxels for i in range(N_TRAIN)]
    assert any(v % 32 for v in voxels), voxels
    return train, val


def _trainer(log_dir, model_seed=11, seed=0, **cfg_kw):
    from csn_amd import CSNTrainer, HRNetSimCSN2S, TrainConfig
    train, val = _collections()
    torch.manual_seed(model_seed)                                                    # the weights, then the dropout seeds of the run
    model = HRNetSimCSN2S(3, N_CLASSES, d_model=64, n_head=2, k_neighbors=1).cuda()
    kw = dict(lr=0.05, optimizer="SGD", scheduler="PolyLR", max_iter=100, batch_size=2, iter_size=2, k_neighbors=1, voxel_size=VOXEL,
              stat_freq=1, log_dir=str(log_dir), model="HRNetSimCSN2S")
    kw.update(cfg_kw)
    return CSNTrainer(model, train, val, TrainConfig(**kw), seed=seed)


def _momentum(trainer):
    state = trainer.optimizer.state_dict()["state"]
    return [(i, state[i]["momentum_buffer"]) for i in sorted(state)]


def test_resume_is_exact(tmp_path):
    """Run A: two epochs in one go.  Run B: one epoch, ``save_checkpoint``, a fresh trainer on a differently initialised model with
    differently seeded generators, ``load_checkpoint``, one more epoch.  The kernels have no floating-point atomics and the dropout
    masks are counter-based, so every parameter, BatchNorm statistic, momentum buffer and the rate are ``torch.equal``."""
    a = _trainer(tmp_path / "a")
    a.construct_graphs(recalculate=False)
    start = {k: v.clone() for k, v in a.model.state_dict().items()}
    loss_a = [a.train_epoch(), a.train_epoch()]

    b1 = _trainer(tmp_path / "b")
    b1.construct_graphs(recalculate=False)
    assert b1.train_neighbors == a.train_neighbors
    loss_b = [b1.train_epoch()]
    path = str(tmp_path / "b" / "mid.pth")
    b1.save_checkpoint(path)
    b2 = _trainer(tmp_path / "b", model_seed=999, seed=5)
    assert not torch.equal(b2.model.head.output.weight, b1.model.head.output.weight)
    b2.load_checkpoint(path)
    loss_b.append(b2.train_epoch())

    assert all(np.isfinite(v) for pair in loss_a for v in pair) and loss_a == loss_b
    sa, sb = a.model.state_dict(), b2.model.state_dict()
    assert list(sa) == list(sb)
    moved = [k for k in sa if not torch.equal(sa[k], start[k])]
    assert any(k.endswith("running_var") for k in moved) and any(k.endswith("kernel") for k in moved) and "head.output.weight" in moved
    assert [k for k in sa if not torch.equal(sa[k], sb[k])] == []
    ma, mb = _momentum(a), _momentum(b2)
    assert len(ma) > 0 and [i for i, _ in ma] == [i for i, _ in mb] and all(torch.equal(x[1], y[1]) for x, y in zip(ma, mb))
    assert a.lr == b2.lr == 0.05 * (1 - 4 / 101) ** 0.9
    assert (a.curr_iter, a.scheduler.last_epoch) == (b2.curr_iter, b2.scheduler.last_epoch) == (5, 4)
    assert a.sampler.state_dict() == b2.sampler.state_dict() and a.sampler.state_dict()["pos"] == 16 - 2 * N_TRAIN
    assert a.aug_rng.bit_generator.state == b2.aug_rng.bit_generator.state


def test_an_iteration_accumulates_iter_size_sub_batches():
    t = _trainer("unused")
    t.construct_graphs(recalculate=False)
    fetched = []
    fetch = t.fetch
    with mock.patch.object(t.optimizer, "step", wraps=t.optimizer.step) as step, \
            mock.patch.object(t, "fetch", side_effect=lambda q: (fetched.append(list(q)), fetch(q))[1]):
        t.model.eval()
        t.train_epoch()
    assert step.call_count == t.iters_per_epoch == 2                                 # ceil(6 / 2 / 2)
    assert t.scheduler.last_epoch == 2 and t.curr_iter == 3
    assert len(fetched) == 4 and all(len(q) == 2 for q in fetched)                   # iter_size sub-batches of batch_size shapes each
    assert sorted(sum(fetched, [])[:N_TRAIN]) == list(range(N_TRAIN))                # the first permutation, then the next one
    assert t.model.training


def test_validate_is_evaluate_on_the_same_fields_and_leaves_the_model_alone():
    from csn_amd import evaluate
    t = _trainer("unused")
    t.construct_graphs(recalculate=False)
    t.train_epoch()
    assert t.model.training
    before = {k: v.clone() for k, v in t.model.state_dict().items()}
    got = t.validate()
    assert t.model.training and all(torch.equal(v, before[k]) for k, v in t.model.state_dict().items())

    train, val = _collections()
    batches = []
    for i in range(N_VAL):
        q = val.batch([i], voxel_size=VOXEL)
        keys = train.neighbor_batches([t.val_neighbors[i]], 1, None, VOXEL)
        batches.append(((q.field(), [k.field() for k in keys]), q.labels))

    def forward_fn(batch):
        field, keys = batch
        return field.interpolate(t.model(field.sparse(), [k.sparse() for k in keys])), field.offsets
    t.model.eval()
    want = evaluate(forward_fn, batches, N_CLASSES, 255)
    assert len(got) == 4 and all(np.isfinite(v) for v in got) and got == want
    assert 0 <= got[1] <= 100 and 0 <= got[2] <= 100 and 0 <= got[3] <= 100


def test_train_rebuilds_the_graph_from_the_best_part_iou_checkpoint(tmp_path):
    """``PatienceState`` is one stalled epoch short of a rebuild and the best Part IoU is out of reach, so the validation after
    epoch 1 — the real one — brings ``should_rebuild()``; ``max_epoch=2`` lets ``train()`` reach it (the last epoch ends without
    one, trainer_csn.py:106-109)."""
    t = _trainer(tmp_path, max_epoch=2)
    t.state.best_val_part_iou, t.state.patience, t.state.cooldown = 1000.0, 1, 1
    t._save_curr_checkpoint("best_part_iou")                                         # the file the rebuild goes back to
    best_file = {k: v.clone() for k, v in t.model.state_dict().items()}
    events, seen = [], {}
    graphs, save = t.construct_graphs, t._save_curr_checkpoint

    def on_graphs(recalculate=False):
        events.append(("graphs", recalculate))
        if recalculate:
            seen["params"] = {k: v.clone() for k, v in t.model.state_dict().items()}
            seen["old"] = (t.train_neighbors, t.val_neighbors)
        graphs(recalculate)
        if recalculate:
            seen["new"] = (t.train_neighbors, t.val_neighbors)

    def on_save(postfix=None):
        events.append(("save", postfix, t.state.n_graph_construction, t.curr_iter))
        save(postfix)
    with mock.patch.object(t, "construct_graphs", side_effect=on_graphs), mock.patch.object(t, "_save_curr_checkpoint", side_effect=on_save):
        t.train()

    plain = [e for e in events if e[0] == "graphs" or e[1] is None]
    assert plain == [("graphs", False), ("save", None, 1, 3), ("graphs", True), ("save", None, 2, 3), ("save", None, 2, 5)]
    assert not any(e[1] == "best_part_iou" for e in events if e[0] == "save")
    # the parameters the new graph was computed with are the file's, not the ones epoch 1 left
    assert all(torch.equal(seen["params"][k], best_file[k]) for k in best_file)
    for (old, new), n_query, same in zip(zip(seen["old"], seen["new"]), (N_TRAIN, N_VAL), (True, False)):
        assert new is not old and [q for q, _ in new] == list(range(n_query))
        assert all(len(nb) == 1 and 0 <= nb[0] < N_TRAIN and not (same and nb[0] == q) for q, nb in new)
    assert (t.train_neighbors, t.val_neighbors) == seen["new"]
    assert (t.state.n_graph_construction, t.state.patience, t.state.cooldown) == (2, 10, 5)
    # resume_optimizer: the rate went back to cfg.lr and a fresh schedule started at iteration 3; epoch 2 stepped it twice
    assert t.scheduler.last_epoch == 3 + 1 + 2 and t.lr == 0.05 * (1 - 6 / 101) ** 0.9
    assert t.model.training and (t.epoch, t.curr_iter) == (2, 5)
    state = torch.load(os.path.join(str(tmp_path), "weights.pth"))
    assert state["csn_data"]["n_graph_construction"] == 2 and state["iteration"] == 5 and state["epoch"] == 3
    assert [(q, list(nb)) for q, nb in state["csn_data"]["train_neighbors"]] == t.train_neighbors


def test_train_resumes_from_its_log_dir_and_ends_where_an_uninterrupted_run_ends(tmp_path):
    """``train()`` to ``max_epoch=1``, then a fresh trainer with ``resume=<log_dir>`` and ``max_epoch=2``, against one ``train()``
    to ``max_epoch=2``: the validations in between draw nothing and update nothing, so the weights are ``torch.equal`` again, and the
    resumed run neither builds a graph nor counts one."""
    a = _trainer(tmp_path / "a", max_epoch=2)
    a.train()
    b1 = _trainer(tmp_path / "b", max_epoch=1)
    b1.train()
    assert (b1.epoch, b1.curr_iter) == (1, 3)
    b2 = _trainer(tmp_path / "b", model_seed=999, seed=5, max_epoch=2, resume=str(tmp_path / "b"))
    with mock.patch.object(b2, "construct_graphs", wraps=b2.construct_graphs) as graphs:
        b2.train()
    assert graphs.call_count == 0 and b2.state.n_graph_construction == a.state.n_graph_construction == 1
    assert (b2.epoch, b2.curr_iter, b2.lr) == (a.epoch, a.curr_iter, a.lr) == (2, 5, 0.05 * (1 - 4 / 101) ** 0.9)
    assert b2.train_neighbors == a.train_neighbors and b2.val_neighbors == a.val_neighbors
    sa, sb = a.model.state_dict(), b2.model.state_dict()
    assert [k for k in sa if not torch.equal(sa[k], sb[k])] == []
    # the run that was interrupted validated its first epoch as a final one; both end on the same last validation
    assert b2.state.best_val_loss_iter in (3, 5) and a.state.best_val_loss_iter in (3, 5)
    fa, fb = torch.load(a.checkpoint_path()), torch.load(b2.checkpoint_path())
    assert (fa["iteration"], fa["epoch"]) == (fb["iteration"], fb["epoch"]) == (5, 3)


def test_command_line_trains_an_epoch_in_a_child_process(tmp_path):
    from csn_amd import HRNetSimCSN2S
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "csn_amd.train_csn", "--synthetic", "6", "--max_epoch", "1",
           "--model", "HRNetSimCSN2S", "--d_model", "64", "--n_head", "2", "--batch_size", "2", "--iter_size", "2", "--k_neighbors", "1",
           "--scheduler", "PolyLR", "--distort_partnet", "True", "--log_dir", str(tmp_path)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    state = torch.load(os.path.join(str(tmp_path), "weights.pth"))
    assert state["iteration"] == 1 + 2 and state["epoch"] == 2 and state["arch"] == "HRNetSimCSN2S"      # 2 iterations ran; the next is 3
    assert state["csn_data"]["n_graph_construction"] == 1 and len(state["csn_data"]["train_neighbors"]) == 6
    model = HRNetSimCSN2S(3, 9, d_model=64, n_head=2, k_neighbors=1)
    model.load_state_dict(state["state_dict"])
    assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
    assert "Current best Part IoU" in res.stdout
