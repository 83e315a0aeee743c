"""The host side of ``SegTrainer``, ``test_split``, the two command lines' test mode and ``collect_partnet_results``
(csn_amd/minkowski_trainer.py, train_csn.py, train_seg.py, collect_partnet_results.py), checked without a GPU: the checkpoint
dictionary and the two ways it loads, the order of events in ``train()`` written out by hand from trainer_seg.py:46-119, the refusals,
the result file byte for byte, and the argument rules."""
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import csn_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFERENCE_KEYS = {"iteration", "epoch", "arch", "state_dict", "optimizer",                                   # utils.py:25-33, no csn_data
                  "best_val_part_iou", "best_val_part_iou_iter", "best_val_shape_iou", "best_val_shape_iou_iter",  # utils.py:34-51
                  "best_val_loss", "best_val_loss_iter", "best_val_acc", "best_val_acc_iter"}
EXTRA_KEYS = {"version", "curr_iter", "scheduler", "augment_rng", "sampler", "torch_rng_state"}


def _split(rng, n):
    from csn_amd import PointCollection
    pts = [rng.standard_normal((20 + i, 3)).astype(np.float32) for i in range(n)]
    return PointCollection(pts, [np.ones(p.shape[0], dtype=np.int32) for p in pts], device="cpu")


def _host_trainer(log_dir, seed=0, **cfg_kw):
    from csn_amd import HRNetSeg2S, SegTrainer, TrainConfig
    rng = np.random.default_rng(5)
    kw = dict(lr=0.1, scheduler="PolyLR", max_iter=50, batch_size=2, log_dir=str(log_dir), model="HRNetSeg2S")
    kw.update(cfg_kw)
    return SegTrainer(HRNetSeg2S(3, 4), _split(rng, 5), _split(rng, 3), TrainConfig(**kw), seed=seed)


# ------------------------------------------------------------------------------------------------------
# the checkpoint dictionary (host tensors: nothing here runs a kernel)
# ------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_and_both_ways_of_loading(tmp_path):
    from tests.test_cpu_hrnet_infer import _reference_named
    torch.manual_seed(1)
    a = _host_trainer(tmp_path, seed=4, k_neighbors=3)                                  # k_neighbors is ignored
    assert a.iters_per_epoch == 3 and a.k_neighbors == 0                                # ceil(5 / 2)
    for _ in range(3):
        next(a.sampler)
    a.spec.draw(2, a.aug_rng)
    for _ in range(2):
        a.optimizer.step()
        a.scheduler.step()
    a.curr_iter, a.epoch = 3, 4
    a.state.record_best(0.7, 55.0, 33.0, 44.0, 3)
    state = a.checkpoint_state()
    assert set(state) == REFERENCE_KEYS | {"csn_amd"} and "csn_data" not in state
    assert set(state["csn_amd"]) == EXTRA_KEYS
    assert (state["iteration"], state["epoch"], state["arch"]) == (3, 5, "HRNetSeg2S")   # epoch + 1, trainer_seg.py:209
    assert a.checkpoint_path() == os.path.join(str(tmp_path), "checkpoint_HRNetSeg2S.pth")
    assert a.checkpoint_path("best_loss").endswith("checkpoint_HRNetSeg2Sbest_loss.pth")
    a._save_curr_checkpoint("best_loss")
    assert not os.path.lexists(os.path.join(str(tmp_path), "weights.pth"))              # only the un-postfixed file is linked
    a._save_curr_checkpoint()
    link = os.path.join(str(tmp_path), "weights.pth")
    assert os.path.islink(link) and os.readlink(link) == "checkpoint_HRNetSeg2S.pth" and os.path.isfile(os.path.join(str(tmp_path), "config.json"))
    torch_state = torch.get_rng_state()

    # 1. with the csn_amd key: every counter and generator continues
    torch.manual_seed(77)
    b = _host_trainer(tmp_path, seed=99)
    b.load_checkpoint(link)
    assert (b.curr_iter, b.epoch) == (3, 5)
    assert all(torch.equal(v, b.model.state_dict()[k]) for k, v in a.model.state_dict().items())
    assert b.state.best_values() == a.state.best_values() and b.state.best_val_part_iou == 33.0
    assert b.scheduler.last_epoch == a.scheduler.last_epoch == 2 and b.lr == a.lr != 0.1
    assert [next(b.sampler) for _ in range(9)] == [next(a.sampler) for _ in range(9)]
    assert np.array_equal(b.spec.draw(3, b.aug_rng).packed(), a.spec.draw(3, a.aug_rng).packed())
    assert torch.equal(torch.get_rng_state(), torch_state)

    # 2. without it, and in the reference's layout: resumed as trainer_seg.py:233-259 does
    del state["csn_amd"]
    state["state_dict"] = _reference_named(state["state_dict"])
    assert not any(k.startswith("backbone.") for k in state["state_dict"])
    bare = os.path.join(str(tmp_path), "bare.pth")
    torch.save(state, bare)
    c = _host_trainer(tmp_path, seed=99)
    c.load_checkpoint(bare)
    assert (c.curr_iter, c.epoch) == (4, 5)                                             # iteration + 1
    assert all(torch.equal(v, c.model.state_dict()[k]) for k, v in a.model.state_dict().items())
    assert c.state.best_val_shape_iou == 44.0 and c.state.best_val_loss_iter == 3
    assert c.scheduler.last_epoch == 4 + 1                                              # a fresh schedule at step curr_iter; torch steps once
    assert c.lr == a.lr                                                                 # the optimizer's own rate is kept
    # resume_optimizer = False: the weights and counters alone
    d = _host_trainer(tmp_path, seed=99, resume_optimizer=False)
    d.load_checkpoint(bare)
    assert (d.curr_iter, d.epoch, d.lr, d.scheduler.last_epoch) == (4, 5, 0.1, 0)
    with pytest.raises(ValueError):
        c.load_checkpoint(os.path.join(str(tmp_path), "missing.pth"))


# ------------------------------------------------------------------------------------------------------
# train(): the order of events, by hand from trainer_seg.py:46-119
# ------------------------------------------------------------------------------------------------------
def _traced(trainer, values):
    """``train()`` with ``train_epoch``, ``validate`` and ``_save_curr_checkpoint`` mocked: the events, and the best values every
    saved file would hold."""
    events, values = [], iter(values)

    def on_epoch():
        events.append(("epoch", trainer.epoch))
        trainer.curr_iter += trainer.iters_per_epoch
        return 0.0, 0.0

    def on_validate():
        events.append(("validate", trainer.model.training))
        return next(values)

    def on_save(postfix=None):
        events.append(("save", postfix, trainer.curr_iter, dict(trainer.state.best_values())))
    with mock.patch.object(trainer, "train_epoch", side_effect=on_epoch), mock.patch.object(trainer, "validate", side_effect=on_validate), \
            mock.patch.object(trainer, "_save_curr_checkpoint", side_effect=on_save), \
            mock.patch.object(trainer.scheduler, "step", wraps=trainer.scheduler.step) as step:
        trainer.train()
    return events, step


def test_train_event_order_and_the_best_files(tmp_path):
    t = _host_trainer(tmp_path, max_epoch=3)
    # (loss, score, part, shape): the second validation ties the Part IoU and the loss (no new best: strict inequalities), raises the
    # Shape IoU and the score; the third improves the loss alone
    vals = [(2.0, 10.0, 5.0, 7.0), (2.0, 11.0, 5.0, 8.0), (1.5, 11.0, 4.0, 8.0)]
    events, step = _traced(t, vals)
    kinds = [e[:2] if e[0] != "validate" else ("validate",) for e in events]
    assert kinds == [("epoch", 1), ("save", None), ("validate",), ("save", "best_part_iou"), ("save", "best_shape_iou"), ("save", "best_loss"),
                     ("save", "best_acc"),
                     ("epoch", 2), ("save", None), ("validate",), ("save", "best_shape_iou"), ("save", "best_acc"),
                     ("epoch", 3), ("validate",), ("save", None), ("save", "best_loss")]
    saves = [e for e in events if e[0] == "save"]
    assert [e[2] for e in saves] == [4] * 5 + [7] * 3 + [10] * 2                        # 3 iterations per epoch, curr_iter starts at 1
    # a best file sees the values moved so far, not the later ones (trainer_seg.py:215-231)
    first = saves[1][3]
    assert first["best_val_part_iou"] == 5.0 and first["best_val_shape_iou"] == 0 and first["best_val_loss"] == float("inf")
    assert saves[0][3]["best_val_part_iou"] == 0                                        # the current file precedes the validation
    assert t.state.best_values() == {"best_val_part_iou": 5.0, "best_val_part_iou_iter": 4, "best_val_shape_iou": 8.0,
                                     "best_val_shape_iou_iter": 7, "best_val_loss": 1.5, "best_val_loss_iter": 10, "best_val_acc": 11.0,
                                     "best_val_acc_iter": 7}
    assert step.call_count == 0                                                         # PolyLR steps inside train_iter, which is mocked
    assert (t.epoch, t.curr_iter) == (3, 10) and t.model.training


def test_max_epoch_one_validates_once_at_the_end(tmp_path):
    t = _host_trainer(tmp_path, max_epoch=1)
    events, _ = _traced(t, [(1.0, 1.0, 1.0, 1.0)])
    assert [e[0] for e in events] == ["epoch", "validate", "save", "save", "save", "save", "save"]
    assert [e[1] for e in events if e[0] == "save"] == [None, "best_part_iou", "best_shape_iou", "best_loss", "best_acc"]


def test_reduce_lr_on_plateau_steps_on_the_validation_loss(tmp_path):
    from torch.optim.lr_scheduler import ReduceLROnPlateau
    t = _host_trainer(tmp_path, max_epoch=3, scheduler="ReduceLROnPlateau")
    assert type(t.scheduler) is ReduceLROnPlateau and t.scheduler.factor == 0.5
    _, step = _traced(t, [(2.0, 1.0, 1.0, 1.0), (3.0, 1.0, 1.0, 1.0), (4.0, 1.0, 1.0, 1.0)])
    assert [c.args for c in step.call_args_list] == [(2.0,), (3.0,)]                    # not after the final validation


def test_resume_loads_weights_pth_of_the_directory(tmp_path):
    a = _host_trainer(tmp_path)
    a.curr_iter, a.epoch = 7, 2
    a._save_curr_checkpoint()
    b = _host_trainer(tmp_path, seed=3, resume=str(tmp_path), max_epoch=3)
    events, _ = _traced(b, [(1.0, 1.0, 1.0, 1.0)])
    assert events[0] == ("epoch", 3) and [e[0] for e in events[:2]] == ["epoch", "validate"]


# ------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------
def test_iter_size_other_than_one_is_refused(tmp_path):
    with pytest.raises(ValueError, match="iter_size"):
        _host_trainer(tmp_path, iter_size=2)


class _Raises(torch.nn.Module):
    def forward(self, *a, **kw):
        raise AssertionError("the model was called")


def test_test_split_refuses_a_non_empty_directory_before_the_model_is_called(tmp_path):
    col = _split(np.random.default_rng(0), 2)
    full = tmp_path / "full"
    full.mkdir()
    (full / "old.txt").write_text("x")
    model = _Raises()
    model.train()
    with pytest.raises(ValueError, match=r"Directory .* not empty\. Please remove the existing prediction\."):
        csn_amd.test_split(model, col, save_pred_dir=str(full))
    assert model.training and os.listdir(str(full)) == ["old.txt"]
    # a missing directory is created before anything else happens; the model here fails after that
    fresh = tmp_path / "a" / "b"
    with pytest.raises(Exception):
        csn_amd.test_split(model, col, save_pred_dir=str(fresh))
    assert fresh.is_dir() and os.listdir(str(fresh)) == []


def test_test_split_needs_the_training_split_for_neighbours():
    from csn_amd import HRNetSimCSN2S
    col = _split(np.random.default_rng(0), 2)
    model = HRNetSimCSN2S(3, 4, d_model=64, n_head=2, k_neighbors=1)
    with pytest.raises(ValueError, match="train_collection"):
        csn_amd.test_split(model, col, k_neighbors=1)
    assert model.training


# ------------------------------------------------------------------------------------------------------
# the result file and its collector
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_iou,part_iou", [(12.345, 67.0), (100.0, 0.0), (33.333333, 45.675)])
def test_results_log_is_byte_equal(tmp_path, shape_iou, part_iou):
    from csn_amd import HRNetSeg2S
    out = tmp_path / "results"
    with mock.patch("csn_amd.minkowski_trainer.evaluate", return_value=(0.5, 90.0, part_iou, shape_iou)) as ev:
        got = csn_amd.test_split(HRNetSeg2S(3, 4), _split(np.random.default_rng(0), 2), save_pred_dir=str(out))
    assert ev.call_count == 1 and got == (0.5, 90.0, part_iou, shape_iou)
    want = "Shape IoU: " + str(np.round(shape_iou, 2)) + "\nPart IoU: " + str(np.round(part_iou, 2))
    assert os.listdir(str(out)) == ["results_log.txt"]
    assert (out / "results_log.txt").read_bytes() == want.encode() and not want.endswith("\n")


def _experiment(base, name, shape_iou, part_iou, evaluation="evaluation"):
    d = base / name / evaluation / "results"
    d.mkdir(parents=True)
    (d / "results_log.txt").write_text(f"Shape IoU: {shape_iou}\nPart IoU: {part_iou}")


def test_collect_results_reads_the_logs_back(tmp_path, capsys):
    from csn_amd.collect_partnet_results import collect_results, main
    _experiment(tmp_path, "Chair-k1-run", 40.5, 30.25)
    _experiment(tmp_path, "Bed-k1-run", 12.35, 67.0, evaluation="best_evaluation")
    _experiment(tmp_path, "Bed-k2-run", 1.0, 2.0)
    (tmp_path / "Bed-k1-run" / "checkpoints").mkdir()                                   # not an *evaluation directory
    assert collect_results(str(tmp_path)) == ([67.0, 2.0, 30.25], [12.35, 1.0, 40.5])   # sorted by experiment
    assert collect_results(str(tmp_path), "1") == ([67.0, 30.25], [12.35, 40.5])
    assert collect_results(str(tmp_path), 2) == ([2.0], [1.0])
    assert main([str(tmp_path), "1"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["PART IOU:", "---------", "[67.0, 30.25]", '=SPLIT("67.0,30.25", ",")',
                     "SHAPE IOU:", "----------", "[12.35, 40.5]", '=SPLIT("12.35,40.5", ",")']
    (tmp_path / "Lamp-k1-run" / "evaluation").mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="Lamp-k1-run.*results_log.txt"):
        collect_results(str(tmp_path), "1")
    assert collect_results(str(tmp_path), "2") == ([2.0], [1.0])


# ------------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------------
def test_train_seg_refuses_an_unknown_argument_before_the_native_library_is_loaded():
    code = ("import runpy, sys\n"
            "sys.argv = ['train_seg', '--synthetic', '6', '--k_neighbors', '1']\n"
            "try:\n"
            "    runpy.run_module('csn_amd.train_seg', run_name='__main__')\n"
            "    rc = 'returned'\n"
            "except SystemExit as e:\n"
            "    rc = e.code\n"
            "from csn_amd import _lib\n"
            "print('RC', rc, 'LOADED', _lib._lib is not None)\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "RC 2 LOADED False" in res.stdout, res.stdout + res.stderr
    assert "unrecognized arguments" in res.stderr
    res = subprocess.run([sys.executable, "-m", "csn_amd.train_seg", "--synthetic", "6", "--is_train", "False"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--weights" in res.stderr                            # test mode without a checkpoint


def test_train_seg_has_the_arguments_of_train_csn_without_the_head(tmp_path):
    from csn_amd import train_csn, train_seg
    names = lambda ap: {a.dest for a in ap._actions}
    assert names(train_csn.build_parser()) - names(train_seg.build_parser()) == {"k_neighbors", "d_model", "n_head"}
    assert names(train_seg.build_parser()) <= names(train_csn.build_parser())
    cfg, args = train_seg.parse_args(["--synthetic", "6", "--log_dir", "x", "--lr", "0.05", "--batch_size", "8", "--max_epoch", "3"])
    assert (cfg.model, cfg.k_neighbors, cfg.lr, cfg.batch_size, cfg.max_epoch, cfg.log_dir) == ("HRNetSeg3S", 0, 0.05, 8, 3, "x")
    assert (args.is_train, args.weights, args.test_files, args.save_pred_dir, args.test_batch_size, args.val_batch_size) == \
        (True, "None", None, None, 1, 1)
    assert train_seg.parse_args(["--synthetic", "6", "--model", "HRNetSeg2S"])[0].model == "HRNetSeg2S"
    for bad in ("HRNetSeg4S", "HRNetSimCSN2S"):
        with pytest.raises(SystemExit):
            train_seg.parse_args(["--synthetic", "6", "--model", bad])
    # the new arguments are the parser's, not the config's: config.json holds what it held
    from csn_amd import TrainConfig
    import dataclasses
    assert not {"is_train", "weights", "test_files", "save_pred_dir", "test_batch_size", "val_batch_size"} & \
        {f.name for f in dataclasses.fields(TrainConfig)}
    cfg, args = train_csn.parse_args(["--synthetic", "6", "--is_train", "1", "--val_batch_size", "2", "--weights", "w.pth"])
    assert (args.is_train, args.val_batch_size, args.weights, cfg.k_neighbors, cfg.model) == (True, 2, "w.pth", 1, "HRNetSimCSN3S")


def _exits(module, argv):
    with pytest.raises(SystemExit) as e:
        module.parse_args(argv)
    return e.value.code


def test_test_mode_data_rules(capsys):
    from csn_amd import train_csn, train_seg
    test = ["--is_train", "False"]
    for module in (train_csn, train_seg):
        assert _exits(module, test + ["--synthetic", "6"]) == 2                                          # no --weights
        assert _exits(module, test + ["--synthetic", "6", "--weights", "None"]) == 2
        assert _exits(module, test + ["--weights", "w.pth"]) == 2                                        # no data
        assert _exits(module, test + ["--weights", "w.pth", "--val_files", "v.h5"]) == 2                 # --val_files is not the test split
        assert _exits(module, test + ["--weights", "w.pth", "--synthetic", "6", "--test_files", "t.h5"]) == 2
        assert _exits(module, test + ["--weights", "w.pth", "--synthetic", "6", "--test_batch_size", "0"]) == 2
        cfg, args = module.parse_args(test + ["--weights", "w.pth", "--synthetic", "6", "--save_pred_dir", "out", "--test_batch_size", "2"])
        assert (args.is_train, args.weights, args.save_pred_dir, args.test_batch_size) == (False, "w.pth", "out", 2)
        # train mode keeps its rule: both splits, or --synthetic
        assert _exits(module, ["--train_files", "a.h5"]) == 2 and _exits(module, ["--test_files", "t.h5"]) == 2
        assert module.parse_args(["--train_files", "a.h5", "--val_files", "v.h5"])[1].val_files == ["v.h5"]
    # HRNetSeg: the test files alone; HRNetSimCSN with neighbours: the training files too, never the validation files
    assert train_seg.parse_args(test + ["--weights", "w.pth", "--test_files", "t.h5"])[1].test_files == ["t.h5"]
    assert _exits(train_csn, test + ["--weights", "w.pth", "--test_files", "t.h5"]) == 2
    assert "--train_files" in capsys.readouterr().err.splitlines()[-1]
    cfg, args = train_csn.parse_args(test + ["--weights", "w.pth", "--test_files", "t.h5", "--train_files", "a.h5", "b.h5"])
    assert (args.train_files, args.val_files, cfg.k_neighbors) == (["a.h5", "b.h5"], None, 1)
    assert train_csn.parse_args(test + ["--weights", "w.pth", "--test_files", "t.h5", "--k_neighbors", "0"])[0].k_neighbors == 0
    # existing refusals stay
    assert _exits(train_csn, ["--synthetic", "6", "--model", "HRNetSimCSN4S"]) == 2
    assert _exits(train_csn, ["--synthetic", "6", "--partnet_category", "Bed-3"]) == 2


def test_synthetic_shapes_are_prefix_stable_and_split_in_three():
    from csn_amd.train_csn import synthetic_shapes, synthetic_split_sizes
    assert synthetic_split_sizes(6, False) == (6, 3, 0) and synthetic_split_sizes(6, True) == (6, 3, 3)
    assert synthetic_split_sizes(5, True) == (5, 3, 3)                                  # N + 2 ceil(N / 2)
    for n, seed in ((6, 123), (5, 0)):
        short = synthetic_shapes(sum(synthetic_split_sizes(n, False)), seed)
        long = synthetic_shapes(sum(synthetic_split_sizes(n, True)), seed)
        assert len(long[0]) == n + 2 * ((n + 1) // 2) == len(short[0]) + (n + 1) // 2
        for kind in (0, 1):
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(short[kind], long[kind]))
        tail = long[0][len(short[0]):]
        assert not any(np.array_equal(t, s) for t in tail for s in short[0] if t.shape == s.shape)       # the test shapes are new ones


def test_num_labels_comes_from_the_checkpoint_in_both_layouts():
    from csn_amd import HRNetSeg2S, HRNetSimCSN2S, checkpoint_num_labels, load_model_state
    from tests.test_cpu_hrnet import _reference_named as csn_named
    from tests.test_cpu_hrnet_infer import _reference_named as seg_named
    torch.manual_seed(0)
    seg, csn = HRNetSeg2S(3, 7), HRNetSimCSN2S(3, 5, d_model=64, n_head=2, k_neighbors=1)
    for model, named, n in ((seg, seg_named, 7), (csn, csn_named, 5)):
        own = model.state_dict()
        ref = named(own)
        assert checkpoint_num_labels(own) == n and checkpoint_num_labels(ref) == n
        flat = {k: (v[0] if k.endswith("output.kernel") or k == "final.3.kernel" else v) for k, v in ref.items()}     # (c_in, c_out)
        assert checkpoint_num_labels(flat) == n
        # ... and either layout loads into a fresh model of that width
        for sd in (own, ref):
            fresh = type(model)(3, n) if model is seg else type(model)(3, n, d_model=64, n_head=2, k_neighbors=1)
            load_model_state(fresh, sd)
            assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in own.items())
    with pytest.raises(ValueError):
        checkpoint_num_labels({"backbone.conv0s1.kernel": torch.zeros(1)})
