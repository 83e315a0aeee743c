"""CPU-side checks of the MinkowskiNet head's loss, metrics and train / test steps (csn_amd/minkowski_training.py, include/csn_hip.h
section 12).  The float64 restatement tests/minkowski_seg_ref.py — the yardstick of the GPU tests — is pinned to goldens that the
reference's own functions produced (tests/golden/g12_minkowski_seg.npz: MinkowskiNet/lib/utils.py and nn.CrossEntropyLoss as
Trainer.test strings them together); SegMeter's finishing arithmetic is run on CPU tensors against the same goldens; the host
pieces (neighbor_batches, load_me_head_state, argument validation) are checked for what they accept and what they refuse.  No
compute call is made here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import minkowski_seg_ref as R

FAKE = 4096          # a non-null, 16-byte aligned "device pointer": every call below must be rejected before it is used


def _eq_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))


def test_golden_holds_the_cases_it_must():
    seqs = R.g12_sequences()
    assert sorted(s["num_labels"] for s in seqs) == [4, 15, 39]
    flags = {"zero": False, "ignored": False, "absent": False, "all_zero_shape": False, "tie": False}
    for s in seqs:
        nl = s["num_labels"]
        for b in s["batches"]:
            t, off, z = b["target"], b["offsets"], b["logits"]
            flags["zero"] |= bool((t == 0).any())
            flags["ignored"] |= bool((t == 255).any())
            for a, e in zip(off, off[1:]):
                flags["all_zero_shape"] |= bool((t[a:e] == 0).all())
                flags["absent"] |= bool(len(set(t[a:e].tolist()) & set(range(1, nl))) not in (0, nl - 1))
            top = z[:, 1:].max(axis=1, keepdims=True)
            flags["tie"] |= bool(((z[:, 1:] == top).sum(axis=1) > 1).any())
    assert all(flags.values()), flags


def test_restatement_equals_the_reference_goldens():
    """Counts exactly; IoUs to 1e-12 (float64 on integers on both sides); precision to 1e-4 absolute on the 0-100 scale (the
    reference forms it in fp32, ulp at 100 = 7.6e-6, a handful of roundings); the loss to 2e-6 relative (torch's fp32
    log-softmax and fp32 mean against float64: the bound tests/test_gpu_loss.py applies to the same arithmetic)."""
    for s in R.g12_sequences():
        nl = s["num_labels"]
        for grouping, final in (("shape", s["final"]), ("batch", s["final_batch"])):
            meter = R.MeterRef(nl)
            for b in s["batches"]:
                off = b["offsets"] if grouping == "shape" else [0, len(b["target"])]
                r = R.seg_ref(b["logits"], b["target"], off, nl)
                assert r["n_bad"] == 0
                assert abs(r["loss"] - b["loss"]) <= 2e-6 * abs(b["loss"])
                assert abs(R.precision_ref(r) - b["prec"]) <= 1e-4
                got = [R.iou_arrays(c) for c in r["counts"]]
                want_i = b["inter"] if grouping == "shape" else b["inter_batch"][None]
                want_u = b["union"] if grouping == "shape" else b["union_batch"][None]
                assert _eq_nan(np.stack([g[0] for g in got]), want_i)
                assert _eq_nan(np.stack([g[1] for g in got]), want_u)
                meter.update(r, len(b["target"]))
            loss, score, part, shape = meter.result()
            assert abs(loss - final[0]) <= 2e-6 * abs(final[0])
            assert abs(score - final[1]) <= 1e-4
            assert abs(part - final[2]) <= 1e-12 and abs(shape - final[3]) <= 1e-12


def test_tie_takes_the_first_class_and_ignored_rows_enter_the_union():
    z = np.zeros((3, 6), dtype=np.float32)
    z[:, 2] = z[:, 4] = 3.0                      # a tie at classes 2 and 4 gives 2
    z[:, 0] = 9.0                                # class 0 is never predicted
    t = np.array([2, 255, 4])
    r = R.seg_ref(z, t, [0, 3], 6)
    assert r["pred"].tolist() == [2, 2, 2]
    assert torch.equal(torch.max(torch.from_numpy(z)[:, 1:], 1)[1] + 1, torch.from_numpy(r["pred"]))
    c = r["counts"][0]
    assert c[2].tolist() == [1, 1, 3]            # the ignored row's prediction is in pr: union = 1 + 3 - 1 = 3, not 2
    assert c[4].tolist() == [0, 1, 0]
    assert r["n_counted"] == 2 and r["n_correct"] == 1


def _batch_from_ref(r):
    from csn_amd.minkowski_training import SegBatch
    stats = torch.tensor([r["loss"], r["n_counted"], r["n_correct"], r["n_bad"]], dtype=torch.float64)
    return SegBatch(torch.from_numpy(r["pred"]).int(), stats, torch.from_numpy(r["counts"]).int())


def test_seg_meter_finishing_arithmetic_against_the_goldens():
    from csn_amd.minkowski_training import SegMeter
    for s in R.g12_sequences():
        nl = s["num_labels"]
        for grouping, final in (("shape", s["final"]), ("batch", s["final_batch"])):
            meter = SegMeter(nl)
            for b in s["batches"]:
                off = b["offsets"] if grouping == "shape" else [0, len(b["target"])]
                meter.update(_batch_from_ref(R.seg_ref(b["logits"], b["target"], off, nl)), len(b["target"]))
            loss, score, part, shape = meter.result()
            assert abs(loss - final[0]) <= 2e-6 * abs(final[0])
            assert abs(score - final[1]) <= 1e-4
            assert abs(part - final[2]) <= 1e-12 and abs(shape - final[3]) <= 1e-12


def test_seg_meter_refuses_bad_labels_and_wrong_widths():
    from csn_amd.minkowski_training import SegMeter
    z = np.random.default_rng(0).standard_normal((10, 4)).astype(np.float32)
    t = np.array([1, 2, 3, 0, 255, 7, 1, 2, 3, 1])                         # 7 is neither a class nor the ignore label
    r = R.seg_ref(z, t, [0, 10], 4)
    assert r["n_bad"] == 1 and r["n_counted"] == 8
    clean = R.seg_ref(np.delete(z, 5, axis=0), np.delete(t, 5), [0, 9], 4)
    assert r["loss"] == clean["loss"] and r["n_correct"] == clean["n_correct"] and np.array_equal(r["counts"], clean["counts"])
    m = SegMeter(4)
    m.update(_batch_from_ref(r), 10)
    with pytest.raises(ValueError, match="labels"):
        m.result()
    with pytest.raises(ValueError):
        SegMeter(5).update(_batch_from_ref(r), 10)
    with pytest.raises(ValueError):
        SegMeter(4).result()


def test_seg_loss_refuses_cpu_tensors():
    from csn_amd import CsnError, seg_loss
    with pytest.raises(CsnError):
        seg_loss(torch.zeros(5, 4), torch.zeros(5, dtype=torch.int64))


def test_public_names_are_exported():
    import csn_amd
    for name in ("seg_loss", "SegBatch", "SegMeter", "train_iter", "evaluate", "neighbor_batches", "load_me_head_state"):
        assert hasattr(csn_amd, name), name


def test_neighbor_batches_restates_get_neighbors():
    from csn_amd.minkowski_training import neighbor_batches
    C = 8
    keys = [torch.full((n, C), float(i)) for i, n in enumerate([3, 5, 2, 7])]
    neighbors = [(0, [2, 1]), (1, [3, 0]), (2, [1, 3])]                    # construct_shape_graph's output, K = 2
    out = neighbor_batches(keys, neighbors, 2)
    assert len(out) == 2
    rows0, off0 = out[0]
    assert off0 == [0, 2, 9, 14] and torch.equal(rows0, torch.cat([keys[2], keys[3], keys[1]]))
    rows1, off1 = out[1]
    assert off1 == [0, 5, 8, 15] and torch.equal(rows1, torch.cat([keys[1], keys[0], keys[3]]))
    assert len(neighbor_batches(keys, neighbors, 1)) == 1
    with pytest.raises(ValueError):
        neighbor_batches(keys, neighbors, 3)
    with pytest.raises(ValueError):
        neighbor_batches(keys, neighbors, 0)


def _me_state(head, kernel_3d, bias_2d):
    sd = {k: torch.randn_like(v) for k, v in head.state_dict().items() if not k.startswith("output.")}
    out_ch, two_c = head.output.weight.shape
    kernel, bias = torch.randn(two_c, out_ch), torch.randn(out_ch)
    sd["output.kernel"] = kernel[None] if kernel_3d else kernel
    sd["output.bias"] = bias[None] if bias_2d else bias
    return sd, kernel, bias


@pytest.mark.parametrize("kernel_3d,bias_2d", [(False, False), (True, True), (True, False)])
def test_load_me_head_state_takes_both_layouts(kernel_3d, bias_2d):
    from csn_amd.minkowski_csn import SimCSNHead
    from csn_amd.minkowski_training import load_me_head_state
    torch.manual_seed(5)
    head = SimCSNHead(32, 2, 6, 1)
    sd, kernel, bias = _me_state(head, kernel_3d, bias_2d)
    sd["backbone.conv1.kernel"] = torch.zeros(3)                           # the rest of the checkpoint is not the head's business
    assert load_me_head_state(head, sd) is head
    assert torch.equal(head.output.weight, kernel.t()) and torch.equal(head.output.bias, bias)
    for name in ("MHA.w_qs.weight", "MHA.fc.weight", "MHA.norm.weight", "MHA.norm.bias", "linear_q.weight", "linear_k.weight"):
        assert torch.equal(head.state_dict()[name], sd[name]), name
    x = torch.randn(4, 64)
    assert torch.allclose(head.output(x), x @ kernel + bias, atol=1e-6)    # a kernel-size-1 convolution on dense rows


def test_load_me_head_state_refusals():
    from csn_amd.minkowski_csn import SimCSNHead
    from csn_amd.minkowski_training import load_me_head_state
    head = SimCSNHead(32, 2, 6, 1)
    before = {k: v.clone() for k, v in head.state_dict().items()}
    good, _, _ = _me_state(head, False, False)
    for key, bad in (("output.kernel", torch.zeros(6, 64)), ("output.kernel", torch.zeros(2, 64, 6)), ("output.kernel", torch.zeros(64, 6, 1)),
                     ("output.bias", torch.zeros(6, 1)), ("output.bias", torch.zeros(7)), ("MHA.fc.weight", torch.zeros(16, 32))):
        with pytest.raises(ValueError):
            load_me_head_state(head, {**good, key: bad})
    for missing in ("output.kernel", "output.bias", "linear_k.weight", "MHA.w_vs.weight"):
        with pytest.raises(ValueError):
            load_me_head_state(head, {k: v for k, v in good.items() if k != missing})
    assert all(torch.equal(v, head.state_dict()[k]) for k, v in before.items())          # a refusal changes nothing
    head0 = SimCSNHead(32, 2, 6, 0)                                                      # no linear_q / linear_k: not asked for
    load_me_head_state(head0, {k: v for k, v in good.items() if not k.startswith("linear_")})


def _ints(*v):
    a = (ctypes.c_int * len(v))(*v)
    return ctypes.cast(a, ctypes.c_void_p).value, a


def test_entry_points_reject_bad_arguments_on_the_host():
    from csn_amd import _lib
    _lib.build()
    L = _lib.lib()
    off, _o = _ints(0, 5, 13)
    short, _s = _ints(0, 5, 12)          # does not end at the row count
    empty, _e = _ints(0, 5, 5)           # an empty segment
    ws = int(L.csn_ragged_seg_workspace_bytes(13))
    assert ws >= 32 and ws % 8 == 0 and L.csn_ragged_seg_workspace_bytes(0) == 0
    def fwd(logits=FAKE, n=13, ld=8, offh=off, segs=2, nc=7, stats=FAKE, w=FAKE, wb=ws):
        return L.csn_ragged_seg_fwd_f32(logits, n, ld, FAKE, offh, FAKE, segs, nc, 255, FAKE, FAKE, FAKE, stats, FAKE, w, wb, None)
    assert fwd(logits=None) == -1
    assert fwd(n=0) == -1
    assert fwd(nc=1) == -1
    assert fwd(ld=6) == -1               # a row shorter than its classes
    assert fwd(offh=None) == -1
    assert fwd(offh=short) == -1
    assert fwd(offh=empty) == -1
    assert fwd(segs=0) == -1
    assert fwd(ld=(1 << 20) + 1) == -5
    assert fwd(stats=FAKE + 4) == -3
    assert fwd(w=FAKE + 4) == -3
    assert fwd(wb=ws - 8) == -6
    def bwd(lse=FAKE, n=13, ld=8, nc=7, dld=7, stats=FAKE):
        return L.csn_ragged_seg_bwd_f32(FAKE, n, ld, FAKE, nc, 255, lse, FAKE, stats, FAKE, FAKE, dld, None)
    assert bwd(lse=None) == -1
    assert bwd(n=-1) == -1
    assert bwd(dld=6) == -1
    assert bwd(ld=6) == -1
    assert bwd(nc=1) == -1
    assert bwd(stats=FAKE + 4) == -3
