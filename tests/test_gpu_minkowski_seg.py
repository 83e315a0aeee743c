"""GPU parity of the MinkowskiNet head's loss, predictions, IoU counts and train / test steps (include/csn_hip.h section 12,
csn_amd/minkowski_training.py): the raw C ABI against the float64 restatement tests/minkowski_seg_ref.py at every row-count,
class-count, pitch and alignment edge; SimCSNHead + seg_loss against the float64 head restatement in both math modes;
evaluate against the reference's goldens; train_iter against manual accumulation; and SegMeter.update without a host sync.

Tolerances are those of tests/test_gpu_loss.py, the same arithmetic (fp32 lse, fp64 sums): loss 2e-6 relative, dlogits
2e-6 x max|ref|; pred and every count EXACTLY.  lse per row (not named by the loss bound) is held to 1e-5 absolute: |lse| <= 16
here, whose ulp is 9.5e-7, and a row is a sum of at most 300 exponentials of a few ulp each, one log1p and one addition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import minkowski_seg_ref as R

pytestmark = pytest.mark.gpu

IGNORE = 255
CANARY = -77.25


@pytest.fixture(scope="module")
def L():
    import csn_amd
    csn_amd.build()
    from csn_amd import _lib
    return _lib


def _segments(rng, N, mode):
    if mode == "one":
        return [0, N]
    if mode == "rows":                                   # every segment one row
        return list(range(N + 1))
    cuts = set(rng.integers(1, N, size=min(N - 1, max(1, N // 300) + 3)).tolist()) if N > 1 else set()
    if N > 5:
        cuts |= {2, 3}                                   # a one-row segment inside
    return [0] + sorted(cuts) + [N]


def _labels(rng, N, nc, ignore):
    lab = rng.integers(1, nc, size=N).astype(np.int64)
    u = rng.random(N)
    lab[u < 0.1] = 0
    if ignore == "some":
        lab[(u > 0.1) & (u < 0.25)] = IGNORE
    elif ignore == "all":
        lab[:] = IGNORE
    return lab


def _logits(rng, N, nc, target):
    z = (2.0 * rng.standard_normal((N, nc))).astype(np.float32)
    rows = np.nonzero((rng.random(N) < 0.5) & (target >= 1) & (target < nc))[0]
    z[rows, target[rows]] += np.float32(3.0)
    if nc > 4:                                           # ties: classes 2 and 4 share the row's maximum
        tie = np.arange(0, N, 7)
        top = z[tie].max(axis=1) + np.float32(0.5)
        z[tie, 2] = top
        z[tie, 4] = top
    inf_rows = np.arange(1, N, 5)                        # -inf logits: probability zero (also as the first class), never the label's
    lab_i = target[inf_rows]
    z[inf_rows[lab_i != 0], 0] = -np.inf
    if nc > 2:
        col = rng.integers(1, nc, size=inf_rows.size)
        col = np.where(col == lab_i, (col % (nc - 1)) + 1, col)
        z[inf_rows, col] = -np.inf
    return z


def _run(L, z, lab, off, nc, ld, dld, shift, grad_out=1.0):
    """logits as an (N, nc) view at pitch ld, `shift` floats into a buffer (shift % 4 != 0: not 16-byte aligned); the padding
    columns of the logits hold 1e30 (they must not be read into any result), those of dlogits a canary."""
    lib = L.lib()
    from csn_amd import functional as CF
    N = z.shape[0]
    dev = torch.device("cuda")
    buf = torch.full((N * ld + shift + 8,), 1e30, device=dev, dtype=torch.float32)
    view = buf[shift:shift + N * ld].view(N, ld)
    view[:, :nc] = torch.from_numpy(z).to(dev)
    dbuf = torch.full((N * dld + shift + 8,), CANARY, device=dev, dtype=torch.float32)
    dview = dbuf[shift:shift + N * dld].view(N, dld)
    labels = torch.from_numpy(lab).to(dev)
    oh = torch.tensor(off, dtype=torch.int32)
    od = oh.to(dev)
    S = len(off) - 1
    lse = torch.full((N,), CANARY, device=dev)
    nll = torch.full((N,), CANARY, device=dev)
    pred = torch.full((N,), -5, device=dev, dtype=torch.int32)
    stats = torch.full((4,), CANARY, device=dev, dtype=torch.float64)
    counts = torch.full((S, nc, 3), -5, device=dev, dtype=torch.int32)
    wb = int(lib.csn_ragged_seg_workspace_bytes(N))
    ws = torch.empty((wb // 8,), device=dev, dtype=torch.float64)
    g = torch.tensor([grad_out], device=dev, dtype=torch.float32)
    L.check(lib.csn_ragged_seg_fwd_f32(view.data_ptr(), N, ld, labels.data_ptr(), oh.data_ptr(), od.data_ptr(), S, nc, IGNORE,
                                       lse.data_ptr(), nll.data_ptr(), pred.data_ptr(), stats.data_ptr(), counts.data_ptr(), ws.data_ptr(), wb,
                                       CF._stream()), "fwd")
    L.check(lib.csn_ragged_seg_bwd_f32(view.data_ptr(), N, ld, labels.data_ptr(), nc, IGNORE, lse.data_ptr(), nll.data_ptr(), stats.data_ptr(),
                                       g.data_ptr(), dview.data_ptr(), dld, CF._stream()), "bwd")
    torch.cuda.synchronize()
    return {"lse": lse.cpu(), "pred": pred.cpu(), "stats": stats.cpu(), "counts": counts.cpu(), "dlogits": dview.cpu(),
            "dbuf": dbuf.cpu(), "shift": shift}


def _compare(got, ref, nc, dld, tag):
    st = got["stats"].numpy()
    assert np.array_equal(got["pred"].numpy().astype(np.int64), ref["pred"]), tag
    assert np.array_equal(got["counts"].numpy().astype(np.int64), ref["counts"]), tag
    assert (st[1], st[2], st[3]) == (ref["n_counted"], ref["n_correct"], ref["n_bad"]), tag
    lse_ref = ref["lse"]
    fin = np.isfinite(lse_ref)
    e_lse = np.abs(got["lse"].numpy().astype(np.float64)[fin] - lse_ref[fin]).max() if fin.any() else 0.0
    assert np.array_equal(got["lse"].numpy()[~fin].astype(np.float64), lse_ref[~fin]), tag
    d = got["dlogits"].numpy().astype(np.float64)
    scale = np.abs(ref["dlogits"]).max()
    e_d = np.abs(d[:, :nc] - ref["dlogits"]).max()
    if ref["n_counted"]:
        e_loss = abs(st[0] - ref["loss"]) / abs(ref["loss"])
    else:
        assert np.isnan(st[0]), tag
        e_loss = 0.0
    print(f"[minkowski_seg] {tag}: loss {e_loss:.1e} lse {e_lse:.1e} dlogits {e_d:.1e} of {scale:.1e}")
    assert e_loss <= 2e-6, tag
    assert e_lse <= 1e-5, tag
    assert e_d <= 2e-6 * scale, tag
    ignored_rows = np.nonzero(np.abs(ref["dlogits"]).max(axis=1) == 0)[0]
    assert (d[ignored_rows][:, :nc] == 0).all(), tag                         # exact zeros, not small numbers
    if dld > nc:                                                             # the padding columns are LEFT UNTOUCHED
        assert (d[:, nc:] == CANARY).all(), tag
    flat = got["dbuf"].numpy()
    n = d.shape[0]
    assert (flat[:got["shift"]] == CANARY).all() and (flat[got["shift"] + n * dld:] == CANARY).all(), tag


@pytest.mark.parametrize("nc", [2, 4, 15, 39, 51])
@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 1301, 40000])
def test_raw_abi_against_float64(L, N, nc):
    rng = np.random.default_rng(1000 * nc + N)
    variants = [  # (ld - nc, dld - nc, shift, segments, ignore)
        (0, 0, 0, "mixed", "some"),                      # contiguous and aligned: the 16-byte forms
        (3, 2, 0, "one", "none"),                        # padded rows
        (0, 0, 1, "mixed", "some"),                      # an unaligned view
        (5, 0, 3, "rows", "some"),                       # unaligned and padded, every segment one row
        (13, 1, 0, "mixed", "none"),                     # ld beyond one staged chunk for the wider class counts
    ]
    for dl, ddl, shift, segs, ign in variants:
        lab = _labels(rng, N, nc, ign)
        z = _logits(rng, N, nc, lab)
        off = _segments(rng, N, segs)
        got = _run(L, z, lab, off, nc, nc + dl, nc + ddl, shift, grad_out=0.75)
        ref = R.seg_ref(z, lab, off, nc, IGNORE, grad_out=0.75)
        _compare(got, ref, nc, nc + ddl, f"N={N} nc={nc} ld=+{dl} dld=+{ddl} shift={shift} {segs} {ign}")


@pytest.mark.parametrize("nc", [59, 60, 130, 300])
def test_wide_class_counts(L, nc):
    """Beyond one staged chunk of columns (59) and beyond the LDS histogram (256 classes): the column-chunk and the
    straight-to-global forms."""
    rng = np.random.default_rng(nc)
    for N, shift, dl in ((700, 0, 0), (129, 2, 1)):
        lab = _labels(rng, N, nc, "some")                # (with 300 classes 255 is BOTH a class and the ignore label: gt counts it)
        z = _logits(rng, N, nc, lab)
        off = _segments(rng, N, "mixed")
        got = _run(L, z, lab, off, nc, nc + dl, nc + dl, shift)
        _compare(got, R.seg_ref(z, lab, off, nc, IGNORE), nc, nc + dl, f"wide nc={nc} N={N}")


def test_all_rows_ignored_gives_nan_and_zero_gradients(L):
    rng = np.random.default_rng(5)
    N, nc = 333, 15
    lab = _labels(rng, N, nc, "all")
    z = _logits(rng, N, nc, lab)
    off = _segments(rng, N, "mixed")
    got = _run(L, z, lab, off, nc, nc, nc, 0)
    assert np.isnan(got["stats"][0].item()) and got["stats"][1].item() == 0
    assert (got["dlogits"] == 0).all()
    _compare(got, R.seg_ref(z, lab, off, nc, IGNORE), nc, nc, "all ignored")


def test_bad_labels_are_counted_and_enter_no_sum(L):
    """A label that is neither the ignore label nor a class: stats[3] counts it; every other result equals the batch without
    those rows (each segment keeps at least one row)."""
    rng = np.random.default_rng(6)
    N, nc = 900, 15
    lab = _labels(rng, N, nc, "some")
    z = _logits(rng, N, nc, lab)
    off = [0, 100, 101, 640, 900]
    bad_rows = np.array([5, 99, 300, 301, 899])
    lab[bad_rows] = [nc, -1, 254, 10 ** 12, nc + 100]
    got = _run(L, z, lab, off, nc, nc, nc, 0)
    ref = R.seg_ref(z, lab, off, nc, IGNORE)
    assert ref["n_bad"] == 5
    _compare(got, ref, nc, nc, "bad labels")
    keep = np.setdiff1d(np.arange(N), bad_rows)
    off2 = [int((keep < o).sum()) for o in off]
    clean = _run(L, z[keep], lab[keep], off2, nc, nc, nc, 0)
    assert clean["stats"][3].item() == 0
    assert torch.equal(clean["counts"], got["counts"])
    assert clean["stats"][1:3].tolist() == got["stats"][1:3].tolist()
    assert abs(clean["stats"][0].item() - got["stats"][0].item()) <= 1e-12 * abs(clean["stats"][0].item())    # other work-group cuts
    assert torch.equal(clean["dlogits"], got["dlogits"][keep]) and torch.equal(clean["pred"], got["pred"][keep])
    assert (got["dlogits"][bad_rows] == 0).all()


def test_two_runs_are_bitwise_equal(L):
    rng = np.random.default_rng(8)
    N, nc = 40000, 39
    lab = _labels(rng, N, nc, "some")
    z = _logits(rng, N, nc, lab)
    off = _segments(rng, N, "mixed")
    a = _run(L, z, lab, off, nc, nc, nc, 0)
    b = _run(L, z, lab, off, nc, nc, nc, 0)
    for k in ("lse", "pred", "stats", "counts", "dlogits"):
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


def test_seg_loss_against_torch_and_strided_logits(L):
    """The autograd surface: loss and gradient against torch's own cross-entropy in float64, on a contiguous tensor and on a
    column slice of a wider one (row pitch > n_classes); pred against torch.max(output[:, 1:], 1)[1] + 1."""
    from csn_amd import seg_loss
    rng = np.random.default_rng(9)
    N, nc = 2500, 39
    lab = _labels(rng, N, nc, "some")
    z = _logits(rng, N, nc, lab)
    t = torch.from_numpy(lab).cuda()
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    want = F.cross_entropy(z64, torch.from_numpy(lab), ignore_index=IGNORE) * 3.0
    want.backward()
    for wide in (False, True):
        base = torch.zeros((N, nc + 9), device="cuda") if wide else None
        x = (base[:, 4:4 + nc].copy_(torch.from_numpy(z)) if wide else torch.from_numpy(z).cuda()).detach().requires_grad_(True)
        loss, sb = seg_loss(x, t, [0, 1000, N], IGNORE)
        (loss * 3.0).backward()
        assert abs(loss.item() * 3.0 - want.item()) <= 2e-6 * abs(want.item())
        gmax = z64.grad.abs().max().item()
        assert (x.grad.cpu().double() - z64.grad).abs().max().item() <= 2e-6 * gmax
        assert torch.equal(sb.pred.cpu().long(), torch.max(torch.from_numpy(z)[:, 1:], 1)[1] + 1)
        assert sb.counts.shape == (2, nc, 3) and sb.counts.is_cuda and sb.stats.is_cuda and sb.pred.is_cuda


# ------------------------------------------------------------------------------------------------------
# the head under the loss, both parity math modes
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
def test_head_with_seg_loss_against_float64(L, mode):
    """SimCSNHead + seg_loss against the float64 head restatement of tests/test_gpu_minkowski_csn.py + float64 cross-entropy:
    every parameter gradient and the input gradients within 1e-4 of each tensor's max, the logits (hence the loss) within 1e-4
    absolute — the bounds that file applies."""
    from tests.test_gpu_minkowski_csn import _head, _pack, _params, _rel, _shape, ref_head
    from csn_amd import seg_loss
    L.check(L.lib().csn_set_math_mode(mode))
    try:
        rng = np.random.default_rng(77)
        qlens, klens, H, C, out_ch = [7, 301, 37], [[37, 5, 1], [64, 130, 7]], 4, 256, 15
        K = len(klens)
        p = _params(rng, H, C, out_ch, K)
        qs = [_shape(rng, n, C) for n in qlens]
        keys = [[_shape(rng, m, C) for m in ms] for ms in klens]
        N = sum(qlens)
        lab = _labels(rng, N, out_ch, "some")
        target = torch.from_numpy(lab)

        head = _head(p, C, H, out_ch, K).eval()
        q, qo = _pack(qs)
        qd = q.cuda().requires_grad_(True)
        kd = [(_pack(ks)[0].cuda().requires_grad_(True), _pack(ks)[1]) for ks in keys]
        loss, sb = seg_loss(head(qd, qo, kd), target.cuda(), qo, IGNORE)
        loss.backward()

        p64 = {n: t.double().requires_grad_(True) for n, t in p.items()}
        q64 = [t.double().requires_grad_(True) for t in qs]
        k64 = [[t.double().requires_grad_(True) for t in ks] for ks in keys]
        ref_logits = ref_head(q64, k64, p64, H, C)
        ref_loss = F.cross_entropy(ref_logits, target, ignore_index=IGNORE)
        ref_loss.backward()

        e = {"dq": _rel(qd.grad, torch.cat([t.grad for t in q64]))}
        for i, ks in enumerate(k64):
            e[f"dk{i}"] = _rel(kd[i][0].grad, torch.cat([t.grad for t in ks]))
        for name, prm in head.named_parameters():
            e[name] = _rel(prm.grad, p64[name].grad)
        e_loss = abs(loss.item() - ref_loss.item())
        print(f"[minkowski_seg] head mode {mode}: loss {e_loss:.1e} " + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
        assert e_loss < 1e-4
        assert max(e.values()) < 1e-4, e
        assert sb.counts.shape == (len(qlens), out_ch, 3) and int(sb.stats[3].item()) == 0
    finally:
        L.lib().csn_set_math_mode(1)


# ------------------------------------------------------------------------------------------------------
# evaluate / train_iter / SegMeter
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_shape", [True, False], ids=["per_shape", "per_batch"])
def test_evaluate_reproduces_the_reference_goldens(L, per_shape):
    """Part and Shape IoU to 1e-9, the loss to 2e-6 relative, the precision to 1e-4 — against the numbers the reference's own
    functions gave (tests/golden/g12_minkowski_seg.npz)."""
    from csn_amd import evaluate
    for s in R.g12_sequences():
        batches = [((torch.from_numpy(b["logits"]).cuda(), b["offsets"]), torch.from_numpy(b["target"])) for b in s["batches"]]
        loss, score, part, shape = evaluate(lambda batch: batch, batches, s["num_labels"], IGNORE, per_shape=per_shape)
        want = s["final"] if per_shape else s["final_batch"]
        print(f"[minkowski_seg] evaluate nl={s['num_labels']} per_shape={per_shape}: {loss} {score} {part} {shape} vs {want.tolist()}")
        assert abs(loss - want[0]) <= 2e-6 * abs(want[0])
        assert abs(score - want[1]) <= 1e-4
        assert abs(part - want[2]) <= 1e-9 and abs(shape - want[3]) <= 1e-9


class _CountingSGD(torch.optim.SGD):
    steps = 0

    def step(self, *a, **k):
        self.steps += 1
        return super().step(*a, **k)


def test_train_iter_equals_manual_accumulation(L):
    """iter_size = 2 on a small head: the accumulated gradients equal two manual F.cross_entropy(..., ignore_index=255) / 2
    backward passes within 1e-4 of each tensor's max (the head's gradient bound), the optimizer and the scheduler step once,
    and the returned loss / precision are the reference's (:209, :221-222)."""
    from tests.test_gpu_minkowski_csn import _head, _pack, _params, _rel, _shape
    from csn_amd import train_iter
    rng = np.random.default_rng(31)
    H, C, out_ch, K = 4, 128, 9, 1
    p = _params(rng, H, C, out_ch, K)
    subs = []
    for qlens, klens in (([40, 9, 75], [33, 120, 5]), ([64, 17], [8, 90])):
        q, qo = _pack([_shape(rng, n, C) for n in qlens])
        k, ko = _pack([_shape(rng, n, C) for n in klens])
        lab = torch.from_numpy(_labels(rng, sum(qlens), out_ch, "some"))
        subs.append(((q.cuda(), qo, [(k.cuda(), ko)]), lab.cuda()))
    a, b = _head(p, C, H, out_ch, K).eval(), _head(p, C, H, out_ch, K).eval()      # eval: no dropout masks, two heads comparable
    before = {n: t.detach().clone() for n, t in a.named_parameters()}
    opt = _CountingSGD(a.parameters(), lr=0.05)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    loss, score = train_iter(lambda batch: (a(batch[0], batch[1], batch[2]), batch[1]), subs, opt, sched)
    assert loss.is_cuda and score.is_cuda and opt.steps == 1 and abs(opt.param_groups[0]["lr"] - 0.025) < 1e-12
    total, last_logits, last_t = 0.0, None, None
    for (q, qo, keys), t in subs:
        last_logits, last_t = b(q, qo, keys), t
        l = F.cross_entropy(last_logits, t, ignore_index=IGNORE) / 2
        total += l.item()
        l.backward()
    e = {n: _rel(t.grad, dict(b.named_parameters())[n].grad.cpu().double()) for n, t in a.named_parameters()}
    print("[minkowski_seg] train_iter " + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
    assert max(e.values()) < 1e-4, e
    assert abs(loss.item() - total) <= 2e-6 * abs(total) + 1e-6
    pred = torch.max(last_logits[:, 1:], 1)[1] + 1
    ok = ((pred == last_t) | (last_t == 0))[last_t != IGNORE]
    assert abs(score.item() - 100.0 * ok.float().mean().item()) <= 1e-4
    for n, t in a.named_parameters():                                        # one SGD step of lr 0.05 on the accumulated gradient
        assert torch.allclose(t.detach(), before[n] - 0.05 * t.grad, rtol=0, atol=1e-6), n


def test_meter_update_makes_no_host_sync(L):
    """torch's sync debug mode, if this build enforces it (probed with a deliberate .item() first); otherwise the weaker
    statement that everything update() holds is a device tensor."""
    from csn_amd import SegMeter, seg_loss
    rng = np.random.default_rng(12)
    nc = 15
    batches = []
    for N in (400, 77, 1301):
        lab = _labels(rng, N, nc, "some")
        loss, sb = seg_loss(torch.from_numpy(_logits(rng, N, nc, lab)).cuda(), torch.from_numpy(lab).cuda(), _segments(rng, N, "mixed"))
        batches.append((sb, N))
    torch.cuda.synchronize()
    probe = torch.ones(3, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            effective = False
        except RuntimeError:
            effective = True
        meter = SegMeter(nc)
        for sb, N in batches:                                                # raises under the mode if update() synchronises
            meter.update(sb, N)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"[minkowski_seg] sync debug mode effective: {effective}")
    assert all(t.is_cuda for t in meter._state.values())
    loss, score, part, shape = meter.result()
    assert all(np.isfinite(v) for v in (loss, score, part, shape)) and 0 <= part <= 100 and 0 <= shape <= 100
