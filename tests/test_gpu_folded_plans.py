"""The folded attention step (tuning.folded_projections, csn_amd/functional.py) on every plan, switch and block edge, against the
float64 restatement of tests/folded_plan_ref.py — the Python that strings the folded kernels together, where
tests/test_gpu_folded.py holds the kernels themselves and the default module step at block 500.

1. every plan of MultiHeadAttention.plan and an irregular one, eval and train (p = 0.1 on both dropouts), at the smallest
   geometries each block edge exists at: the folded run AND the unfolded run (same seed) each within 1e-4 of the reference tensor's
   max-abs on xhat, sums, dW_q, dW_k, dW_v, dW_fc — the project's contract (tests/test_gpu_folded.py part 4).  Nothing tighter is
   asserted between the two forms.  Slot ranges ("cross_only"), unwritten query slots ("cross", irregular), one 32-key tile, a
   second tile of 4 keys, a full query tile, short last blocks.
2. the switches that stay live under the fold, one at a time on the train plan: still folded, the intended launches, float64 at
   1e-4, and against the default run the same bits where the project claims them (grouped_fwd, kv_same, tile_major_scores), 2e-4
   of max-abs otherwise (the TOL of tests/test_gpu_module.py::test_fused_data_flow_equals_the_unfused_one).
3. the linked mix under the fold — W_fv^T travelling through the link into the mix's own LayerNorm backward — with default
   switches, fused_mix_bwd off, link_mix off, and the two-phase step (CrossShapeAt._csa_cm_overlapped) with and without
   descriptor reuse: logits and all 11 gradients against the float64 oracle with the step's own masks.
4. a plan the fold declines (values from another slot than the keys) keeps the bits of the switched-off step.

Every case asserts through the call hook which form ran."""
import numpy as np
import pytest
import torch

from oracle import csa_oracle as orc
from tests import folded_plan_ref as fr
from tests.test_gpu_folded import _masked_oracle
from tests.test_gpu_mix_fold import _train_step

pytestmark = pytest.mark.gpu
TOL = 2e-4                                              # of tests/test_gpu_module.py::test_fused_data_flow_equals_the_unfused_one
W_NAMES = ("w_qs", "w_ks", "w_vs", "fc")
FOLD_ONLY, UNFOLDED_DKV = ("csn_fold_weights_f32", "csn_tile_planes_f32", "csn_unfold_wgrads_f32"), "csn_block_attn_bwd_dkv_f32"


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _bf16x3(L):
    L.check(L.lib().csn_set_math_mode(1))
    yield
    L.set_call_hook(None)
    L.lib().csn_dev_set(L.DEV_KV_SAME, 1)
    L.lib().csn_set_thread_score_layout(0)
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


class _Recorded:
    """The launching library calls (name, the thread's score layout at the call), the seeds drawn through CF.draw_seeds and the
    queries for the out-projection's sums workspace made inside the block."""

    def __init__(self, L):
        self.L, self.calls, self.layouts, self.seeds, self.ws_queries = L, [], {}, [], 0

    def __enter__(self):
        from csn_amd import functional as CF
        lib = self.L.lib()
        self._draw, self._ws = CF.draw_seeds, lib.csn_outproj_ln_workspace_floats

        def hook(name, phase):
            if phase == "begin":
                self.calls.append(name)
                self.layouts.setdefault(name, set()).add(lib.csn_get_thread_score_layout())

        def draw(n):
            s = self._draw(n)
            self.seeds.append(s)
            return s

        def ws(*a):
            self.ws_queries += 1
            return self._ws(*a)

        CF.draw_seeds, lib.csn_outproj_ln_workspace_floats = draw, ws
        self.L.set_call_hook(hook)
        return self

    def __exit__(self, *exc):
        from csn_amd import functional as CF
        self.L.set_call_hook(None)
        CF.draw_seeds, self.L.lib().csn_outproj_ln_workspace_floats = self._draw, self._ws


def _assert_form(calls, folded, what=""):
    if folded:
        assert all(n in calls for n in FOLD_ONLY) and UNFOLDED_DKV not in calls, f"{what}: the step did not fold"
        assert "csn_block_attn_bwd_dv_scores_f32" not in calls
    else:
        assert not any(n in calls for n in FOLD_ONLY) and UNFOLDED_DKV in calls, f"{what}: the step folded"


# ---- att.evaluate on a plan ---------------------------------------------------------------------------------------------------
def _evaluate(L, kind, T, x_all, w, R, Rs, train, fold, **switches):
    """-> ({xhat, sums, dw_q, dw_k, dw_v, dw_fc} on the CPU, the _Recorded of the step, the plan)"""
    from csn_amd import tuning
    from csn_amd.csa_models import MultiHeadAttention
    N = x_all.shape[2]
    att = MultiHeadAttention(1, fr.C, fr.C, fr.C, block=T, n_blocks=None)
    for n in W_NAMES:
        getattr(att, n).weight.data.copy_(w[n])
    att = att.cuda().train(train)
    assert att.dropout_rates() == ((fr.P_DROP, fr.P_DROP) if train else (0.0, 0.0))
    plan = fr.make_plan(att, kind, torch.device("cuda"))
    xd, Rd, Rsd = x_all.cuda(), R.cuda(), Rs.cuda()
    assert not xd.requires_grad                                  # (input gradients wanted: the fold is declined)
    torch.manual_seed(fr.STEP_SEED)
    with _Recorded(L) as rec, tuning.override(folded_projections=fold), tuning.override(**switches):
        xhat, sums = att.evaluate(xd, plan, att.geometry(n_points=N), want_sums=True)
        loss = (xhat * Rd).sum() + (sums * Rsd).sum()
        grads = torch.autograd.grad(loss, [getattr(att, n).weight for n in W_NAMES])
        torch.cuda.synchronize()
    got = dict(zip(fr.TENSORS, [t.detach().cpu() for t in (xhat, sums) + tuple(grads)]))
    return got, rec, plan


_runs, _refs = {}, {}


def _case_run(L, kind, T, N, train, fold):
    """the default-switch run of a case, made once"""
    key = (kind, T, N, train, fold)
    if key not in _runs:
        c = fr.case(kind, T, N)
        _runs[key] = _evaluate(L, kind, T, c["x_all"], c["w"], c["R"], c["Rs"], train, fold)
    return _runs[key]


def _reference(kind, T, N, train, seeds):
    key = (kind, T, N, train)
    if key not in _refs:
        _refs[key] = fr.reference(fr.case(kind, T, N), train, seeds)
    return _refs[key]


def _hold_to_float64(got, ref, tag):
    r = fr.ratios(got, ref)
    print(f"[folded-plans] {tag}: " + " ".join(f"{n} {v:.2e}" for n, v in r.items()))
    return {n: v for n, v in r.items() if not v <= 1e-4}


CASES = fr.gpu_cases()


@pytest.mark.parametrize("kind,T,N,train", CASES, ids=[f"{k}-T{T}-N{N}-{'train' if tr else 'eval'}" for k, T, N, tr in CASES])
def test_every_plan_folded_and_unfolded_against_float64(L, kind, T, N, train):
    c = fr.case(kind, T, N)
    runs = {fold: _case_run(L, kind, T, N, train, fold) for fold in (True, False)}
    seeds = None
    for fold, (got, rec, plan) in runs.items():
        _assert_form(rec.calls, fold, f"fold={fold}")
        assert (plan.E, plan.S) == (c["E"], c["S"])
        assert rec.seeds == ([fr.step_seeds()] if train else []), "the step drew other seeds than the reference's masks"
        if fold:
            n_q, n_kv = len(plan.q_ranges or [0]), len(plan.kv_ranges or [0])
            assert rec.calls.count("csn_tile_planes_f32") == n_kv and rec.calls.count("csn_block_attn_bwd_dq_f32") == 1
            # Q'' of the plan's query ranges; dM range by range (+ the W_fv gradient inside the LayerNorm backward call)
            assert rec.calls.count("csn_project_f32") == n_q and rec.calls.count("csn_project_wgrad_f32") == n_q
        seeds = rec.seeds[0] if train else None
    ref = _reference(kind, T, N, train, seeds)
    missed = {}
    for fold, (got, rec, plan) in runs.items():
        form = "folded" if fold else "unfolded"
        bad = _hold_to_float64(got, ref, f"{kind} T={T} N={N} {'train' if train else 'eval'} {form}")
        if bad:
            missed[form] = bad
    assert not missed, missed


# ---- 2. switches under the fold ----------------------------------------------------------------------------------------------
SWITCHES = [("grouped_dq", False, False), ("grouped_fwd", False, True), ("kv_same", False, True), ("tile_major_scores", True, True),
            ("fused_point_sums", False, False)]                 # (switch, value, the same bits as the default run)


@pytest.mark.parametrize("T,N", [(36, 100), fr.BIG], ids=lambda v: str(v))
@pytest.mark.parametrize("switch,value,same_bits", SWITCHES, ids=[f"{s}={v}" for s, v, _ in SWITCHES])
def test_switches_under_the_fold(L, switch, value, same_bits, T, N):
    kind = "csa_train"
    c = fr.case(kind, T, N)
    base, base_rec, plan = _case_run(L, kind, T, N, True, True)
    got, rec, _ = _evaluate(L, kind, T, c["x_all"], c["w"], c["R"], c["Rs"], True, True, **{switch: value})
    _assert_form(base_rec.calls, True, "default")
    _assert_form(rec.calls, True, f"{switch}={value}")
    assert rec.seeds == base_rec.seeds == [fr.step_seeds()]
    lib = L.lib()
    dq, fwd, fwd_g = "csn_block_attn_bwd_dq_f32", "csn_block_attn_fwd_f32", "csn_block_attn_fwd_grouped_f32"
    assert base_rec.calls.count(dq) == 1 and base_rec.calls.count(fwd_g) == 1 and fwd not in base_rec.calls
    assert base_rec.ws_queries == 1 and base_rec.layouts[dq] == base_rec.layouts[fwd_g] == {0}
    if switch == "grouped_dq":
        assert len(plan.dq_colors) == 4 and rec.calls.count(dq) == 4          # a query shape serves K + 1 mixed + its pooled evaluation
    else:
        assert rec.calls.count(dq) == 1
    if switch == "grouped_fwd":
        assert rec.calls.count(fwd) == 1 and fwd_g not in rec.calls
    else:
        assert rec.calls.count(fwd_g) == 1 and fwd not in rec.calls
    if switch == "kv_same":
        assert lib.csn_dev_get(L.DEV_KV_SAME) == 0                           # (set before the dQ launch, process-wide)
    if switch == "tile_major_scores":
        want = int((lib.csn_attn_bwd_grouping(fr.C, T) & 19) == 19)
        assert want == 1 or T != 500                                         # (the 500-key block has the tile-major instances)
        assert rec.layouts[fwd_g] == rec.layouts[dq] == {want}
    else:
        assert rec.layouts[dq] == {0}
    assert rec.ws_queries == (0 if switch == "fused_point_sums" else 1)      # off: no per-tile partials, sums by a streaming pass
    bad = _hold_to_float64(got, _reference(kind, T, N, True, rec.seeds[0]), f"{kind} T={T} N={N} train {switch}={value}")
    assert not bad, bad
    for n in fr.TENSORS:
        if same_bits:
            assert torch.equal(got[n].view(torch.int32), base[n].view(torch.int32)), n
        else:
            err, scale = (got[n] - base[n]).abs().max().item(), base[n].abs().max().item()
            print(f"[folded-plans]   {switch}={value} {n}: {err / scale:.2e} of max-abs from the default run")
            assert err <= TOL * scale, n


# ---- 3. the linked mix under the fold ------------------------------------------------------------------------------------------
MIX_T, MIX_N = 36, 100
MIX_VARIANTS = {"default": {}, "fused_mix_bwd-off": dict(fused_mix_bwd=False), "link_mix-off": dict(link_mix=False),
                "two-phase": {}, "two-phase-reuse": {}}
_mix = {}


def _mix_case():
    if "case" not in _mix:
        _mix["case"] = orc.conditioned_csa_case(np.random.default_rng(9100), fr.B, fr.K, 1, fr.N_CLS, 4.0, 2.0, 1.0, n_points=MIX_N)
    return _mix["case"]


class _Ready:
    """A neighbour stack that has already arrived, in the form CrossShapeAt._csa_cm_overlapped takes.  reuse: the neighbours'
    pooled descriptors come from gather_pooled — here a separate (folded) "self" evaluation of the neighbour maps, which is what
    their owners would have run."""

    def __init__(self, model, stack, reuse):
        self.model, self.stack, self.reuse_descriptors = model, stack, reuse

    def wait(self):
        return self.stack

    def gather_pooled(self, own):
        att, (b, k1, c, n) = self.model.attention, self.stack.shape
        nbrs = self.stack[:, 1:].reshape(b * (k1 - 1), c, n).contiguous()
        _, sums = att.evaluate(nbrs, att.plan("self", b * (k1 - 1), 1, nbrs.device), att.geometry(n_points=n), want_sums=True)
        return (sums / n).view(b, k1 - 1, c)


def _two_phase_step(m, x, nb, lab, reuse):
    from csn_amd import functional as CF
    stack = nb.squeeze(-1).contiguous()                                    # (B, K + 1, C, N), slot 0 = the shape itself
    with CF.math_mode(m.attention.math_mode):
        logits = m._logits(m._csa_cm_overlapped(stack[:, 0].contiguous(), _Ready(m, stack, reuse)))
    loss = orc.masked_ce_loss(logits, lab)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.item(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}


def _two_phase_masks(seeds, reuse):
    """The two-phase step draws one seed pair per evaluate call and numbers the evaluations per call: phase 1 ("self2") [b] mixed
    self, [B + b] pooled self; phase 2 ("csa_cross") [b*K + k-1] mixed cross, [B*K + b*K + k-1] neighbour self — with descriptor
    reuse ("cross_only") the mixed cross ones alone, and the neighbours' self evaluations [b*K + k-1] are a third call.  The masks
    of the calls stacked behind each other, and the oracle's calls mapped into that numbering."""
    B, K = fr.B, fr.K
    sizes = (2 * B, B * K, B * K) if reuse else (2 * B, 2 * B * K)
    assert len(seeds) == len(sizes)
    sets = [fr.masks(E, MIX_T, MIX_N, s) for E, s in zip(sizes, seeds)]
    am, fm = torch.cat([s[0] for s in sets]), torch.cat([s[1] for s in sets])
    o2 = 2 * B
    nbr0 = o2 + B * K                                                      # first neighbour-self evaluation in either form

    def evals_of(call):
        if call == 0:
            return [B + b for b in range(B)]
        if call <= K:
            return [nbr0 + b * K + call - 1 for b in range(B)]
        if call == K + 1:
            return list(range(B))
        return [o2 + b * K + (call - K - 1) - 1 for b in range(B)]

    return (am, fm), evals_of


def _mix_reference(seeds, variant):
    p, x, nb, lab = _mix_case()
    key = (variant if variant.startswith("two-phase") else "one-call", tuple(map(tuple, seeds)))
    if key not in _mix:
        n_blocks = (MIX_N + MIX_T - 1) // MIX_T
        if variant.startswith("two-phase"):
            masks, evals_of = _two_phase_masks(seeds, variant.endswith("reuse"))
            kw = dict(seeds=None, masks=masks, evals_of=evals_of)
        else:
            assert len(seeds) == 1
            kw = dict(seeds=seeds[0])
        _mix[key] = tuple(_masked_oracle(p, x, nb, lab, dt, MIX_T, n_blocks, fr.B, fr.K, p_drop=fr.P_DROP, **kw)
                          for dt in (torch.float64, torch.float32))
    return _mix[key]


@pytest.mark.parametrize("variant", list(MIX_VARIANTS))
def test_linked_mix_under_the_fold_against_float64(L, variant):
    """Logits and each of the 11 gradients within 1e-4 of the float64 oracle's max-abs (the step's own masks); the four
    compatibility-head tensors with _grad_check's noise term, 10 x the deviation of the same oracle in fp32 from float64."""
    from csn_amd import tuning
    from csn_amd.csa_models import get_model
    p, x, nb, lab = _mix_case()
    m = get_model("csa", fr.N_CLS, 1, fr.K, block=MIX_T, n_blocks=None)
    m.load_state_dict(p, strict=False)
    m = m.cuda().train(True)
    torch.manual_seed(fr.STEP_SEED)
    with _Recorded(L) as rec, tuning.override(**MIX_VARIANTS[variant]):
        if variant.startswith("two-phase"):
            logits, loss, grads = _two_phase_step(m, x.cuda(), nb.cuda(), lab.cuda(), variant.endswith("reuse"))
        else:
            logits, loss, grads = _train_step(m, x.cuda(), nb.cuda().contiguous(), lab.cuda())
    calls = rec.calls
    _assert_form(calls, True, variant)
    lnb, mix_bwd, ln_bwd = "csn_outproj_lnb_f32", "csn_mix_bwd_f32", "csn_outproj_ln_bwd_f32"
    if variant in ("default", "two-phase", "two-phase-reuse"):
        assert lnb in calls and mix_bwd not in calls                        # the mix ran the mixed evaluations' LayerNorm backward
    else:
        assert mix_bwd in calls and lnb not in calls and ln_bwd in calls
    n_eval = {"two-phase": 2, "two-phase-reuse": 3}.get(variant, 1)         # evaluate calls, each folded
    n_planes = {"two-phase-reuse": 1 + fr.K + 1}.get(variant, n_eval)       # ("cross_only": one call per key / value slot range)
    assert calls.count("csn_fold_weights_f32") == calls.count("csn_unfold_wgrads_f32") == n_eval == len(rec.seeds)
    assert calls.count("csn_tile_planes_f32") == n_planes
    (r_logits, r_loss, r_grads), ref32 = _mix_reference(rec.seeds, variant)
    assert len(grads) == 11
    logits = logits.cpu()
    missed = {}
    e_log = (logits.double() - r_logits).abs().max().item() / r_logits.abs().max().item()
    print(f"[folded-plans] mix {variant}: logits {e_log:.2e} loss {abs(loss - r_loss):.2e}")
    if not e_log <= 1e-4:
        missed["logits"] = e_log
    if not abs(loss - r_loss) <= 1e-5:
        missed["loss"] = abs(loss - r_loss)
    for n, g in grads.items():
        r = r_grads[n].double()
        scale = r.abs().max().item()
        noise = (ref32[2][n].double() - r).abs().max().item() if n.startswith("compatibility") else 0.0
        err = (g.cpu().double() - r).abs().max().item()
        print(f"[folded-plans]   {n}: {err / scale:.2e} of max-abs (allowed {1e-4 + 10.0 * noise / scale:.2e})")
        if not err <= 1e-4 * scale + 10.0 * noise:
            missed[n] = (err / scale, 1e-4 + 10.0 * noise / scale)
    assert not missed, missed


# ---- 4. a declined plan keeps its bits -----------------------------------------------------------------------------------------
def test_plan_with_shifted_values_is_declined_and_keeps_its_bits(L):
    """plan("qkv"): the values live B slots after the keys (v_shift = B), K = V = x does not hold — the unfolded calls run whatever
    the switch says"""
    T, N = 36, 100
    x_all, c = fr.case("csa", T, N)["x_all"], fr.case("cross", T, N)            # 3 B slots; B evaluations
    outs = {}
    for fold in (True, False):
        got, rec, plan = _evaluate(L, "qkv", T, x_all, c["w"], c["R"], c["Rs"], True, fold)
        assert plan.v_shift == fr.B and (plan.E, plan.S) == (fr.B, 3 * fr.B)
        _assert_form(rec.calls, False, f"fold={fold}")
        outs[fold] = got
    for n in fr.TENSORS:
        assert torch.isfinite(outs[True][n]).all()
        assert torch.equal(outs[True][n].view(torch.int32), outs[False][n].view(torch.int32)), n
