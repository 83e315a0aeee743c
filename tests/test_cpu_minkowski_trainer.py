"""The host side of the MinkowskiNet CSN trainer (csn_amd/minkowski_solvers.py, minkowski_trainer.py, train_csn.py), checked without
a GPU: the schedules against their closed forms, ``PatienceState`` against traces written out by hand from trainer_csn.py:114-158,
``InfSampler``, the checkpoint dictionary's keys and the two ways it loads, and the command line's refusal of an unknown argument."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------
# optimizer and schedules
# ------------------------------------------------------------------------------------------------------
def _lrs(cfg, steps=13):
    from csn_amd.minkowski_solvers import initialize_optimizer, initialize_scheduler
    opt = initialize_optimizer([torch.nn.Parameter(torch.zeros(1))], cfg)
    sched = initialize_scheduler(opt, cfg)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out, sched


@pytest.mark.parametrize("name", ["PolyLR", "SquaredLR", "ExpLR"])
def test_lambda_schedules_equal_their_closed_forms(name):
    """Steps 0..12 with max_iter = 10: the polynomial ones reach 0 at s = 11 and leave the reals at s = 12 (a negative base to the
    power 0.9), exactly as the formula says; ``abs`` compares either kind of number."""
    from csn_amd.minkowski_solvers import TrainConfig
    cfg = TrainConfig(lr=0.1, scheduler=name, max_iter=10, poly_power=0.9, exp_step_size=4, exp_gamma=0.9)
    closed = {"PolyLR": lambda s: (1 - s / (10 + 1)) ** 0.9, "SquaredLR": lambda s: (1 - s / (10 + 1)) ** 2,
              "ExpLR": lambda s: 0.9 ** (s / 4)}[name]
    lrs, _ = _lrs(cfg)
    for s, lr in enumerate(lrs):
        want = 0.1 * closed(s)
        assert abs(lr - want) <= 1e-12 * abs(want), (name, s, lr, want)
    assert len(lrs) == 13 and lrs[0] == 0.1


def test_torch_schedules_and_optimizers_get_their_arguments():
    from torch.optim.lr_scheduler import ReduceLROnPlateau, StepLR
    from csn_amd.minkowski_solvers import TrainConfig, initialize_optimizer, initialize_scheduler
    p = [torch.nn.Parameter(torch.zeros(1))]
    cfg = TrainConfig(lr=0.2, scheduler="StepLR", step_size=3, step_gamma=0.25)
    lrs, sched = _lrs(cfg, 7)
    assert type(sched) is StepLR and sched.step_size == 3 and sched.gamma == 0.25
    assert lrs == pytest.approx([0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.0125], rel=1e-12)
    opt = initialize_optimizer(p, TrainConfig(scheduler="ReduceLROnPlateau"))
    sched = initialize_scheduler(opt, TrainConfig(scheduler="ReduceLROnPlateau"), factor=0.3, patience=7, cooldown=9)
    assert type(sched) is ReduceLROnPlateau and (sched.factor, sched.patience, sched.cooldown) == (0.3, 7, 9)

    sgd = initialize_optimizer(p, TrainConfig(lr=0.3, sgd_momentum=0.8, sgd_dampening=0.2, weight_decay=1e-3))
    g = sgd.param_groups[0]
    assert type(sgd) is torch.optim.SGD and (g["lr"], g["momentum"], g["dampening"], g["weight_decay"]) == (0.3, 0.8, 0.2, 1e-3)
    adam = initialize_optimizer(p, TrainConfig(optimizer="Adam", lr=0.01, adam_beta1=0.7, adam_beta2=0.95, weight_decay=1e-2))
    g = adam.param_groups[0]
    assert type(adam) is torch.optim.Adam and (g["lr"], g["betas"], g["weight_decay"]) == (0.01, (0.7, 0.95), 1e-2)
    with pytest.raises(ValueError):
        initialize_optimizer(p, TrainConfig(optimizer="RMSProp"))
    with pytest.raises(ValueError):
        initialize_scheduler(sgd, TrainConfig(scheduler="CosineLR"))


def test_a_schedule_continues_at_a_given_step_and_its_state_round_trips():
    from csn_amd.minkowski_solvers import TrainConfig, initialize_optimizer, initialize_scheduler
    cfg = TrainConfig(lr=0.1, scheduler="PolyLR", max_iter=100)
    lrs, sched = _lrs(cfg, 6)
    opt = initialize_optimizer([torch.nn.Parameter(torch.zeros(1))], cfg)
    fresh = initialize_scheduler(opt, cfg)
    fresh.load_state_dict(sched.state_dict())
    assert fresh.last_step == sched.last_step == 6
    opt.step()
    fresh.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(0.1 * (1 - 7 / 101) ** 0.9, rel=1e-12)
    # last_step = s: torch steps once when it builds a schedule, so the rate is the one of s + 1 (as in trainer_csn.py:147-148)
    opt = initialize_optimizer([torch.nn.Parameter(torch.zeros(1))], cfg)
    initialize_scheduler(opt, cfg, last_step=40)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.1 * (1 - 41 / 101) ** 0.9, rel=1e-12)


def test_train_config_restates_the_reference_defaults():
    from csn_amd.minkowski_solvers import TrainConfig
    c = TrainConfig()
    assert (c.lr, c.optimizer, c.sgd_momentum, c.sgd_dampening, c.weight_decay, c.adam_beta1, c.adam_beta2) == (1e-2, "SGD", 0.9, 0.1, 1e-4, 0.9, 0.999)
    assert (c.scheduler, c.max_iter, c.poly_power, c.step_size, c.step_gamma, c.exp_step_size, c.exp_gamma) == ("StepLR", 60000, 0.9, 10000, 0.5, 445, 0.99)
    assert (c.max_epoch, c.iter_size, c.batch_size, c.k_neighbors, c.ignore_label, c.voxel_size, c.stat_freq) == (200, 1, 16, 1, 255, 0.05, 40)
    assert (c.resume, c.resume_optimizer, c.log_dir) == (None, True, "outputs/default")


# ------------------------------------------------------------------------------------------------------
# PatienceState: every expected trace below is written out by hand from trainer_csn.py:114-158
# ------------------------------------------------------------------------------------------------------
def _epoch(st, part_iou, it=0):
    st.observe(part_iou)
    st.record_best(1.0, 0.0, part_iou, 0.0, it)
    return st.cooldown, st.patience


def test_patience_constants_and_a_monotone_rise_never_rebuild():
    from csn_amd import minkowski_trainer as T
    assert (T.MAX_PATIENCE, T.MAX_COOLDOWN, T.MAX_GRAPH_CONSTRUCTION) == (10, 5, 3)
    st = T.PatienceState(k_neighbors=1)
    st.constructed()
    assert (st.patience, st.cooldown, st.n_graph_construction) == (10, 5, 1)
    for e in range(1, 21):
        cooldown, patience = _epoch(st, float(e))
        assert (cooldown, patience) == (5 - e, 10) and not st.should_rebuild()         # cooldown is clamped only on the falling branch
    assert st.n_graph_construction == 1 and st.best_val_part_iou == 20.0


def test_patience_on_a_plateau_cooldown_first_then_patience_then_one_rebuild_and_the_cap():
    from csn_amd.minkowski_trainer import PatienceState
    st = PatienceState(k_neighbors=2)
    st.constructed()
    trace = [_epoch(st, 50.0)] + [_epoch(st, 50.0) for _ in range(12)]
    assert trace == [(4, 10), (3, 10), (2, 10), (1, 10), (0, 9), (0, 8), (0, 7), (0, 6), (0, 5), (0, 4), (0, 3), (0, 2), (0, 1)]
    assert not st.should_rebuild()
    assert _epoch(st, 49.0) == (0, 0) and st.should_rebuild()                          # epoch 14, not one sooner
    st.rebuilt()
    assert (st.patience, st.cooldown, st.n_graph_construction) == (10, 5, 2) and not st.should_rebuild()
    # the second plateau costs 4 + 10 epochs again; a new best in between only refills patience, cooldown keeps running
    assert [_epoch(st, 50.0) for _ in range(5)] == [(4, 10), (3, 10), (2, 10), (1, 10), (0, 9)]
    assert _epoch(st, 51.0) == (-1, 10)
    assert [_epoch(st, 51.0) for _ in range(10)] == [(0, 9 - i) for i in range(10)]
    assert st.should_rebuild()
    st.rebuilt()
    assert st.n_graph_construction == 3
    # MAX_GRAPH_CONSTRUCTION reached: patience stops falling, cooldown is no longer clamped
    assert [_epoch(st, 0.0) for _ in range(8)] == [(4, 10), (3, 10), (2, 10), (1, 10), (0, 10), (-1, 10), (-2, 10), (-3, 10)]
    assert not st.should_rebuild()


def test_patience_never_falls_without_neighbours():
    from csn_amd.minkowski_trainer import PatienceState
    st = PatienceState(k_neighbors=0)
    assert [_epoch(st, 0.0) for _ in range(7)] == [(4, 10), (3, 10), (2, 10), (1, 10), (0, 10), (-1, 10), (-2, 10)]
    st.patience = 0
    assert not st.should_rebuild()


def test_best_values_move_in_the_reference_order_and_carry_the_iteration():
    from csn_amd.minkowski_trainer import PatienceState
    st = PatienceState(1)
    assert st.best_values() == {"best_val_part_iou": 0, "best_val_part_iou_iter": 0, "best_val_shape_iou": 0, "best_val_shape_iou_iter": 0,
                                "best_val_loss": float("inf"), "best_val_loss_iter": 0, "best_val_acc": 0, "best_val_acc_iter": 0}
    seen = []

    def on_best(postfix):
        seen.append((postfix, dict(st.best_values())))
    assert st.record_best(2.0, 10.0, 5.0, 7.0, 3, on_best) == ["best_part_iou", "best_shape_iou", "best_loss", "best_acc"]
    # the file written for the first best value does not know the later ones yet (trainer_csn.py:331-346)
    assert seen[0][1]["best_val_part_iou"] == 5.0 and seen[0][1]["best_val_shape_iou"] == 0 and seen[0][1]["best_val_loss"] == float("inf")
    assert seen[2][1]["best_val_loss"] == 2.0 and seen[2][1]["best_val_acc"] == 0
    assert st.record_best(1.5, 9.0, 5.0, 8.0, 5) == ["best_shape_iou", "best_loss"]     # equal Part IoU is no new best
    assert st.best_values() == {"best_val_part_iou": 5.0, "best_val_part_iou_iter": 3, "best_val_shape_iou": 8.0, "best_val_shape_iou_iter": 5,
                                "best_val_loss": 1.5, "best_val_loss_iter": 5, "best_val_acc": 10.0, "best_val_acc_iter": 3}


# ------------------------------------------------------------------------------------------------------
# InfSampler
# ------------------------------------------------------------------------------------------------------
def test_inf_sampler_blocks_are_permutations_and_its_state_restores():
    from csn_amd.minkowski_trainer import InfSampler
    n = 7
    a, b = InfSampler(n, True, np.random.default_rng(3)), InfSampler(n, True, np.random.default_rng(3))
    assert len(a) == n
    draws = [next(a) for _ in range(5 * n)]
    blocks = [draws[i * n:(i + 1) * n] for i in range(5)]
    assert all(sorted(blk) == list(range(n)) for blk in blocks) and len({tuple(blk) for blk in blocks}) > 1
    assert [next(b) for _ in range(5 * n)] == draws
    for _ in range(3):                                                                 # mid-permutation
        next(a)
    state = a.state_dict()
    assert state["pos"] == 3 and sorted(state["perm"]) == list(range(n))
    ahead = [next(a) for _ in range(2 * n)]
    c = InfSampler(n, True, np.random.default_rng(999))
    c.load_state_dict(state)
    assert [next(c) for _ in range(2 * n)] == ahead
    plain = InfSampler(3, False)
    assert [next(plain) for _ in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    with pytest.raises(ValueError):
        InfSampler(4, False).load_state_dict(state)
    with pytest.raises(ValueError):
        InfSampler(4, True)


# ------------------------------------------------------------------------------------------------------
# the checkpoint dictionary (host tensors: nothing here runs a kernel)
# ------------------------------------------------------------------------------------------------------
REFERENCE_KEYS = {"iteration", "epoch", "arch", "state_dict", "optimizer", "csn_data",                       # utils.py:25-33
                  "best_val_part_iou", "best_val_part_iou_iter", "best_val_shape_iou", "best_val_shape_iou_iter",  # utils.py:34-51
                  "best_val_loss", "best_val_loss_iter", "best_val_acc", "best_val_acc_iter"}
CSN_DATA_KEYS = {"patience", "cooldown", "n_graph_construction", "train_neighbors", "val_neighbors"}        # trainer_csn.py:318-322
EXTRA_KEYS = {"version", "curr_iter", "scheduler", "augment_rng", "graph_rng", "sampler", "torch_rng_state"}


def _host_trainer(log_dir, seed=0, **cfg_kw):
    from csn_amd import CSNTrainer, HRNetSimCSN2S, PointCollection, TrainConfig
    rng = np.random.default_rng(5)
    def split(n):
        pts = [rng.standard_normal((20 + i, 3)).astype(np.float32) for i in range(n)]
        return PointCollection(pts, [np.ones(p.shape[0], dtype=np.int32) for p in pts], device="cpu")
    cfg = TrainConfig(lr=0.1, scheduler="PolyLR", max_iter=50, batch_size=2, iter_size=2, k_neighbors=1, log_dir=str(log_dir),
                      model="HRNetSimCSN2S", **cfg_kw)
    model = HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=1)
    return CSNTrainer(model, split(5), split(3), cfg, seed=seed)


def test_checkpoint_keys_and_both_ways_of_loading(tmp_path):
    from tests.test_cpu_hrnet import _reference_named
    torch.manual_seed(1)
    a = _host_trainer(tmp_path, seed=4)
    assert a.iters_per_epoch == 2                                                       # ceil(5 / 2 / 2)
    a.construct_graphs(recalculate=False)
    a.state.constructed()
    assert [q for q, _ in a.train_neighbors] == list(range(5)) and all(nb != [q] and 0 <= nb[0] < 5 for q, nb in a.train_neighbors)
    assert [q for q, _ in a.val_neighbors] == list(range(3)) and all(0 <= nb[0] < 5 for _, nb in a.val_neighbors)
    # some history: a few draws of every generator, two scheduler steps, a best value, a falling patience
    for _ in range(3):
        next(a.sampler)
    a.spec.draw(2, a.aug_rng)
    for _ in range(2):
        a.optimizer.step()
        a.scheduler.step()
    a.curr_iter, a.epoch = 3, 4
    a.state.record_best(0.7, 55.0, 33.0, 44.0, 3)
    a.state.patience, a.state.cooldown = 6, 0
    state = a.checkpoint_state()
    assert set(state) == REFERENCE_KEYS | {"csn_amd"}
    assert set(state["csn_data"]) == CSN_DATA_KEYS and set(state["csn_amd"]) == EXTRA_KEYS
    assert (state["iteration"], state["epoch"], state["arch"]) == (3, 5, "HRNetSimCSN2S")            # epoch + 1, trainer_csn.py:323
    path = a.checkpoint_path()
    assert path == os.path.join(str(tmp_path), "checkpoint_HRNetSimCSN2S.pth")
    assert a.checkpoint_path("best_part_iou").endswith("checkpoint_HRNetSimCSN2Sbest_part_iou.pth")
    a._save_curr_checkpoint()
    link = os.path.join(str(tmp_path), "weights.pth")
    assert os.path.islink(link) and os.readlink(link) == "checkpoint_HRNetSimCSN2S.pth" and os.path.isfile(os.path.join(str(tmp_path), "config.json"))
    torch_state = torch.get_rng_state()

    # 1. with the csn_amd key: every counter and generator continues
    torch.manual_seed(77)
    b = _host_trainer(tmp_path, seed=99)
    b.load_checkpoint(link)
    assert (b.curr_iter, b.epoch) == (3, 5)
    assert all(torch.equal(v, b.model.state_dict()[k]) for k, v in a.model.state_dict().items())
    assert b.train_neighbors == a.train_neighbors and b.val_neighbors == a.val_neighbors
    assert (b.state.patience, b.state.cooldown, b.state.n_graph_construction) == (6, 0, 1)
    assert b.state.best_values() == a.state.best_values()
    assert b.scheduler.last_epoch == a.scheduler.last_epoch == 2 and b.lr == a.lr != 0.1
    assert [next(b.sampler) for _ in range(9)] == [next(a.sampler) for _ in range(9)]
    assert np.array_equal(b.spec.draw(3, b.aug_rng).packed(), a.spec.draw(3, a.aug_rng).packed())
    assert b.graph_rng.integers(0, 1 << 30, 4).tolist() == a.graph_rng.integers(0, 1 << 30, 4).tolist()
    assert torch.equal(torch.get_rng_state(), torch_state)

    # 2. without it (a checkpoint of the reference's): accepted, resumed as trainer_csn.py:348-387 does
    del state["csn_amd"]
    state["state_dict"] = _reference_named(state["state_dict"])                         # ... and in the reference's layout
    bare = os.path.join(str(tmp_path), "bare.pth")
    torch.save(state, bare)
    c = _host_trainer(tmp_path, seed=99)
    c.load_checkpoint(bare)
    assert (c.curr_iter, c.epoch) == (4, 5)                                             # iteration + 1
    assert all(torch.equal(v, c.model.state_dict()[k]) for k, v in a.model.state_dict().items())
    assert c.train_neighbors == a.train_neighbors and c.state.patience == 6 and c.state.best_val_part_iou == 33.0
    assert c.lr == a.lr                                                                 # the optimizer's own rate is kept
    # the saved state_dict itself is the model's: plain load_state_dict takes it
    fresh = _host_trainer(tmp_path).model
    fresh.load_state_dict(torch.load(path)["state_dict"])
    with pytest.raises(ValueError):
        c.load_checkpoint(os.path.join(str(tmp_path), "missing.pth"))


def test_k_neighbors_zero_saves_no_graph(tmp_path):
    from csn_amd import CSNTrainer, HRNetSimCSN2S, PointCollection, TrainConfig
    pts = [np.zeros((4, 3), dtype=np.float32)] * 3
    col = PointCollection(pts, [np.ones(4, dtype=np.int32)] * 3, device="cpu")
    t = CSNTrainer(HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=0), col, col, TrainConfig(k_neighbors=0, log_dir=str(tmp_path)))
    assert set(t.checkpoint_state()) == (REFERENCE_KEYS - {"csn_data"}) | {"csn_amd"}
    with pytest.raises(ValueError):
        t.construct_graphs()
    with pytest.raises(ValueError):
        CSNTrainer(HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=0), col, col, TrainConfig(k_neighbors=1))


# ------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------
def test_cli_refuses_an_unknown_argument_before_the_native_library_is_loaded():
    code = ("import runpy, sys\n"
            "sys.argv = ['train_csn', '--synthetic', '6', '--partnet_category', 'Bed-3']\n"
            "try:\n"
            "    runpy.run_module('csn_amd.train_csn', run_name='__main__')\n"
            "    rc = 'returned'\n"
            "except SystemExit as e:\n"
            "    rc = e.code\n"
            "from csn_amd import _lib\n"
            "print('RC', rc, 'LOADED', _lib._lib is not None)\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "RC 2 LOADED False" in res.stdout, res.stdout + res.stderr
    assert "unrecognized arguments" in res.stderr
    res = subprocess.run([sys.executable, "-m", "csn_amd.train_csn", "--max_epoch", "1"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--synthetic" in res.stderr                          # no data named


def test_cli_maps_its_arguments_onto_the_config():
    from csn_amd.train_csn import parse_args, synthetic_shapes
    cfg, args = parse_args(["--synthetic", "6", "--log_dir", "x", "--model", "HRNetSimCSN2S", "--k_neighbors", "2", "--lr", "0.5e-1",
                            "--optimizer", "Adam", "--batch_size", "8", "--scheduler", "ReduceLROnPlateau", "--max_epoch", "3",
                            "--resume_optimizer", "False", "--iter_size", "2", "--stat_freq", "7"])
    assert (cfg.log_dir, cfg.model, cfg.k_neighbors, cfg.lr, cfg.optimizer, cfg.batch_size, cfg.scheduler, cfg.max_epoch) == \
        ("x", "HRNetSimCSN2S", 2, 0.05, "Adam", 8, "ReduceLROnPlateau", 3)
    assert (cfg.resume_optimizer, cfg.iter_size, cfg.stat_freq, cfg.resume, cfg.weight_decay) == (False, 2, 7, None, 1e-4)
    assert args.synthetic == 6 and args.seed == 123 and args.distort_partnet is False
    with pytest.raises(SystemExit):
        parse_args(["--synthetic", "6", "--model", "HRNetSimCSN4S"])
    pts, labs = synthetic_shapes(9, 0)
    counts = [p.shape[0] for p in pts]
    assert len(set(counts)) > 1 and all(150 <= c <= 260 for c in counts)
    assert all(p.dtype == np.float32 and l.shape == (p.shape[0],) and 1 <= l.min() and l.max() <= 8 for p, l in zip(pts, labs))
