"""The attention step, call for call: every launching library call of a forward + backward with its arguments, and the sha256
of every result — one text file that must not change under a host-only refactor of csn_amd/functional.py.

    python scripts/trace_step_calls.py OUT.txt [--full]     (on the MI355X; run on two trees, then compare the files byte for byte)

Only the public surface is used (MultiHeadAttention.evaluate / plan, EvalPlan, get_model, tuning.override, math_mode,
_lib.lib(), _lib._SIGNATURES), so the one file runs unchanged on any revision.

Every entry-point attribute of ``_lib.lib()`` is wrapped around a case.  A line is written for each call that takes a stream
(i.e. launches) and for csn_dev_set (process-wide state a launch depends on): the name, the thread's math mode / act16 format /
score layout at the call, every non-pointer argument in ``repr``, every pointer as 0 (null) or a letter by order of first
appearance within the call (so "k == v" shows, addresses do not).  Pure host queries (predicates, workspace sizes, the getters
and the per-thread setters themselves) are not written: WHEN a predicate is asked is not part of the step, what the launches
see of the thread state is, and that is on every line.  After a case: the sha256 of every output and gradient.
--full writes all of these lines; without it a case is ONE line (its number of calls and the sha256 over their lines, its number
of results and the sha256 over their digest lines) — what differs between two trees shows all the same, and --full then says where.
Both forms end with the tally of the whole run: calls per entry point, the csn_block_attn_bwd_dq_f32 calls by (probs_tiles, with
group offsets), the launches by thread state.

Cases: C = d = 256 at the geometries of tests/folded_plan_ref.py (every plan kind, the irregular and the ranged plan, train and
eval, the four math modes, every switch _MHAEvals reads flipped alone with and without the fold, input gradients, v_shift = 1),
the 500-key block for the instances that exist only there (dV from the scores, tile-major scores), narrower heads for the
recompute / flash flows and each forced score flow, and the linked mix through CrossShapeAt."""
import collections
import hashlib
import os
import sys
from ctypes import c_void_p

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from csn_amd import _lib, tuning                                   # noqa: E402
from csn_amd import functional as CF                                # noqa: E402
from csn_amd.csa_models import MultiHeadAttention, get_model        # noqa: E402
from oracle import csa_oracle as orc                                # noqa: E402
from tests import folded_plan_ref as fr                             # noqa: E402

MODES = ("fp32", "bf16x3", "bf16", "fp16")
SWITCHES = [("kv_tiles", False), ("fused_point_sums", False), ("grouped_dkv", False), ("grouped_dq", False), ("grouped_fwd", False),
            ("tile_major_scores", True), ("qkv_one_pass", True), ("dv_from_scores", False), ("kv_same", False), ("wg64", False)]
MIX_SWITCHES = [("link_mix", False), ("fused_mix_bwd", False), ("act16", False)]
FLOWS = (tuning.KEEP_SCORES, tuning.RECOMPUTE_DQ, tuning.FLASH)


class Trace:
    def __init__(self, out, full):
        self.out, self.full, self.lib, self.lines = out, full, _lib.lib(), []
        self.by_name, self.dq_forms, self.by_state = (collections.Counter() for _ in range(3))
        self.names = [n for n in _lib._SIGNATURES if hasattr(self.lib, n)]
        self.orig = {n: getattr(self.lib, n) for n in self.names}

    def _wrap(self, name):
        fn, argtypes = self.orig[name], _lib._SIGNATURES[name][1]
        written = name == "csn_dev_set" or (bool(argtypes) and argtypes[-1] is c_void_p and name != "csn_status_string")

        def call(*a):
            if written:
                seen, parts = {}, []
                for v, t in zip(a, argtypes):
                    if t is c_void_p:
                        v = getattr(v, "value", v)
                        parts.append("0" if not v else seen.setdefault(v, chr(ord("a") + len(seen))))
                    else:
                        parts.append(repr(v))
                state = (self.orig["csn_get_math_mode"](), self.orig["csn_get_thread_act16"](), self.orig["csn_get_thread_score_layout"]())
                self.lines.append(f"  {name} mode/act16/layout={state} ({', '.join(parts)})\n")
                self.by_name[name] += 1
                if name != "csn_dev_set":
                    self.by_state[state] += 1
                if name == "csn_block_attn_bwd_dq_f32":
                    self.dq_forms[(a[-4], "offsets" if a[-3] else "no offsets")] += 1
            return fn(*a)
        return call

    def case(self, title, step):
        """step() -> {name: tensor}; launches inside are written, then the digests"""
        self.lines = []
        for n in self.names:
            setattr(self.lib, n, self._wrap(n))
        try:
            torch.manual_seed(fr.STEP_SEED)
            results = step()
            torch.cuda.synchronize()
        except _lib.CsnError as e:
            results = {}
            self.lines.append(f"  raised CsnError: {e}\n")
        finally:
            for n in self.names:
                setattr(self.lib, n, self.orig[n])
        digests = [f"  sha256 {k} {tuple(t.shape)} " + hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
                   + "\n" for k, t in results.items()]
        if self.full:
            self.out.write(f"== {title}\n" + "".join(self.lines + digests))
        else:
            sha = lambda ls: hashlib.sha256("".join(ls).encode()).hexdigest()
            self.out.write(f"== {title} | {len(self.lines)} calls {sha(self.lines)} | {len(digests)} results {sha(digests)}\n")
        self.out.flush()

    def tally(self):
        for title, counter in (("calls per entry point", self.by_name), ("csn_block_attn_bwd_dq_f32 by (probs_tiles, group offsets)",
                                                                         self.dq_forms), ("launches by (math mode, act16, score layout)", self.by_state)):
            self.out.write(f"== {title}\n" + "".join(f"  {k}: {n}\n" for k, n in sorted(counter.items(), key=repr)))


def evaluate_step(kind, T, N, train, mode, H=1, d=fr.C, C=fr.C, want_dx=False, B=fr.B):
    """forward + backward of att.evaluate on a plan -> xhat, sums and the gradients"""
    rng = np.random.default_rng(4200 + 13 * T + N + 101 * H + d)
    att = MultiHeadAttention(H, C, d, d, block=T, n_blocks=None, math=mode)
    for lin in (att.w_qs, att.w_ks, att.w_vs, att.fc):
        lin.weight.data.copy_(torch.from_numpy(rng.standard_normal(tuple(lin.weight.shape)).astype(np.float32) / np.sqrt(lin.weight.shape[1])))
    att = att.cuda().train(train)
    dev = torch.device("cuda")
    if kind == "irregular":
        plan = CF.EvalPlan(np.array(fr.IRREGULAR[0]), np.array(fr.IRREGULAR[1]), fr.IRREGULAR[2], dev)
    else:
        plan = att.plan(kind, B, fr.PLAN_K1.get(kind, fr.K1), dev)
    x = torch.from_numpy(rng.standard_normal((plan.S, C, N)).astype(np.float32)).cuda().requires_grad_(want_dx)
    R = torch.from_numpy(rng.standard_normal((plan.E, C, N)).astype(np.float32)).cuda()
    Rs = torch.from_numpy(rng.standard_normal((plan.E, C)).astype(np.float32)).cuda()

    def step():
        xhat, sums = att.evaluate(x, plan, att.geometry(n_points=N), want_sums=True)
        wanted = [att.w_qs.weight, att.w_ks.weight, att.w_vs.weight, att.fc.weight] + ([x] if want_dx else [])
        grads = torch.autograd.grad((xhat * R).sum() + (sums * Rs).sum(), wanted)
        return dict(zip(("xhat", "sums", "dw_q", "dw_k", "dw_v", "dw_fc", "dx"), (xhat, sums) + tuple(grads)))
    return step


def model_step(T, N, train, mode):
    """CrossShapeAt "csa" forward + loss + backward (the linked mix) -> logits and the parameter gradients"""
    p, x, nb, lab = orc.conditioned_csa_case(np.random.default_rng(9100 + T), fr.B, fr.K, 1, fr.N_CLS, 4.0, 2.0, 1.0, n_points=N)
    m = get_model("csa", fr.N_CLS, 1, fr.K, block=T, n_blocks=None)
    m.load_state_dict(p, strict=False)
    m = m.cuda().train(train)
    m.attention.math_mode = CF.mode_id(mode)
    x, nb, lab = x.cuda(), nb.cuda().contiguous(), lab.cuda()

    def step():
        m.zero_grad(set_to_none=True)
        logits = m(x, "train" if train else "test", nb)
        orc.masked_ce_loss(logits, lab).backward()
        out = {"logits": logits}
        out.update({k: q.grad for k, q in m.named_parameters() if q.grad is not None})
        return out
    return step


def main(path, full=False):
    assert torch.cuda.is_available(), "the trace needs the MI355X"
    with open(path, "w") as out:
        tr = Trace(out, full)
        T, N = 36, 100
        # every plan kind, train / eval, default mode; "qkv" with B = 1 is v_shift = 1
        for kind in fr.PLANS + ("qkv",):
            for train in (False, True):
                for Tg, Ng in (fr.SMALL if kind == "csa_train" else ((T, N),)):
                    tr.case(f"evaluate {kind} T={Tg} N={Ng} train={train}", evaluate_step(kind, Tg, Ng, train, "bf16x3"))
        tr.case("evaluate qkv B=1 (v_shift = 1)", evaluate_step("qkv", T, N, True, "bf16x3", B=1))
        tr.case("evaluate qkv B=1 (v_shift = 1) fp32", evaluate_step("qkv", T, N, True, "fp32", B=1))
        for fold in (True, False):
            with tuning.override(folded_projections=fold):
                # the four math modes on the train plan and the ranged plan, input gradients
                for mode in MODES:
                    for kind in ("csa_train", "cross_only"):
                        tr.case(f"evaluate {kind} {mode} fold={fold}", evaluate_step(kind, T, N, True, mode))
                    tr.case(f"evaluate csa_train {mode} fold={fold} dx", evaluate_step("csa_train", T, N, True, mode, want_dx=True))
                tr.case(f"evaluate cross_only bf16x3 fold={fold} dx", evaluate_step("cross_only", T, N, True, "bf16x3", want_dx=True))
                # every switch alone: the small block, and the 500-key block (dV from the scores, tile-major, grouped dK / dV)
                for name, value in SWITCHES:
                    for Tg, Ng in ((T, N), fr.BIG):
                        with tuning.override(**{name: value}):
                            tr.case(f"evaluate csa_train T={Tg} fold={fold} {name}={value}", evaluate_step("csa_train", Tg, Ng, True, "bf16x3"))
                tr.case(f"evaluate csa_train T=500 fold={fold}", evaluate_step("csa_train", *fr.BIG, True, "bf16x3"))
                tr.case(f"evaluate cross_only T=500 fold={fold}", evaluate_step("cross_only", *fr.BIG, True, "bf16x3"))
                tr.case(f"evaluate csa_train T=500 bf16 fold={fold}", evaluate_step("csa_train", *fr.BIG, True, "bf16"))
                # the linked mix through CrossShapeAt
                for mode in MODES:
                    for train in (False, True):
                        tr.case(f"model csa {mode} train={train} fold={fold}", model_step(T, N, train, mode))
                for name, value in MIX_SWITCHES:
                    for mode in ("bf16x3", "bf16", "fp16"):
                        with tuning.override(**{name: value}):
                            tr.case(f"model csa {mode} fold={fold} {name}={value}", model_step(T, N, True, mode))
                for mode in ("bf16x3", "bf16", "fp16"):          # (bf16 / fp16: the grouped dK / dV instances, hence bf16 gradient maps)
                    tr.case(f"model csa {mode} T=500 fold={fold}", model_step(*fr.BIG, True, mode))
        # a block past 512 keys: the single-product modes run as bf16x3 on fp32 maps
        for mode in ("bf16x3", "bf16"):
            tr.case(f"evaluate csa_train T=600 {mode}", evaluate_step("csa_train", 600, 640, True, mode))
        # narrower heads: the configured flows (flash / recompute) and each flow forced, per mode
        for H, d in ((2, 64), (2, 96), (2, 128), (4, 32)):
            for mode in MODES:
                tr.case(f"evaluate csa_train H={H} d={d} {mode}", evaluate_step("csa_train", T, N, True, mode, H=H, d=d, C=128))
        for flow in FLOWS:
            with tuning.override(score_flow={1: flow, 2: flow}):
                for mode in ("bf16x3", "bf16", "fp16"):
                    tr.case(f"evaluate csa_train H=2 d=64 {mode} flow={flow}", evaluate_step("csa_train", T, N, True, mode, H=2, d=64, C=128))
                    tr.case(f"evaluate csa_train d=256 {mode} flow={flow}", evaluate_step("csa_train", T, N, True, mode))
                    for name in ("grouped_dq", "grouped_dkv"):
                        with tuning.override(**{name: False}):
                            tr.case(f"evaluate csa_train H=2 d=64 {mode} flow={flow} {name}=False",
                                    evaluate_step("csa_train", T, N, True, mode, H=2, d=64, C=128))
                    tr.case(f"model csa {mode} flow={flow}", model_step(T, N, True, mode))
        tr.tally()


if __name__ == "__main__":
    main(sys.argv[1], "--full" in sys.argv[2:])
