"""tests/folded_plan_ref.py, the float64 reference of tests/test_gpu_folded_plans.py, checked where no GPU is needed:

1. conditioning — the same restatement in float32 stays within 1e-5 of the float64 one (of each tensor's max-abs: a tenth of the
   1e-4 contract the kernels are held to) for EVERY (plan, geometry, mode) the GPU test uses.  A condition on the inputs: a case
   that misses it is a badly conditioned case, and the case is what has to change;
2. algebra — the folded association (M = W_k^T W_q / t, W_fv = W_fc W_v) in float64 agrees with the reference to 1e-12;
3. the tie to the oracle — for the "self" plan without masks the reference is orc.mha_blockdiag before the affine."""
import pytest
import torch

from oracle import csa_oracle as orc
from tests import folded_plan_ref as fr

CASES = fr.gpu_cases()
IDS = [f"{plan}-T{T}-N{N}-{'train' if train else 'eval'}" for plan, T, N, train in CASES]

_ref64 = {}


def _reference(plan, T, N, train):
    key = (plan, T, N, train)
    if key not in _ref64:
        _ref64[key] = fr.reference(fr.case(plan, T, N), train)
    return _ref64[key]


def test_plan_table_is_the_modules_own():
    table = fr.plan_table()
    assert set(table) == set(fr.PLANS)
    q, kv, S = table["cross_only"]
    assert (q, kv, S) == ([0, 0, 3, 3], [1, 2, 4, 5], 6)                  # B = 2, K = 2: own slots b * 3, neighbours b * 3 + k
    q, kv, S = table["csa_train"]
    assert len(q) == 12 and S == 6 and q[-2:] == [0, 3] and kv[-2:] == [0, 3]
    assert table["cross"] == ([0, 1], [2, 3], 4) and table["self2"] == ([0, 1, 0, 1], [0, 1, 0, 1], 2)
    assert table["irregular"] == fr.IRREGULAR
    assert 1 not in table["irregular"][0]                                 # a slot nobody queries


def test_step_seeds_are_what_draw_seeds_draws():
    from csn_amd import functional as CF
    state = torch.get_rng_state()
    try:
        torch.manual_seed(fr.STEP_SEED)
        assert CF.draw_seeds(2) == fr.step_seeds()
    finally:
        torch.set_rng_state(state)


@pytest.mark.parametrize("plan,T,N,train", CASES, ids=IDS)
def test_float32_restatement_stays_within_a_tenth_of_the_contract(plan, T, N, train):
    c = fr.case(plan, T, N)
    assert c["x_all"].shape == (c["S"], fr.C, N) and c["R"].shape == (c["E"], fr.C, N)
    r = fr.ratios(fr.reference(c, train, dtype=torch.float32), _reference(plan, T, N, train))
    print(f"[plan-ref] {plan} T={T} N={N} train={train}: " + " ".join(f"{n} {v:.2e}" for n, v in r.items()))
    for n, v in r.items():
        assert v <= 1e-5, (n, v)


@pytest.mark.parametrize("plan,T,N,train", CASES, ids=IDS)
def test_folded_association_is_the_same_function(plan, T, N, train):
    r = fr.ratios(fr.reference(fr.case(plan, T, N), train, association="folded"), _reference(plan, T, N, train))
    print(f"[plan-ref] {plan} T={T} N={N} train={train} folded: " + " ".join(f"{n} {v:.2e}" for n, v in r.items()))
    for n, v in r.items():
        assert v <= 1e-12, (n, v)


def test_masks_reach_the_reference():
    """another seed gives other masks and a materially different result: the train-mode cases above are train-mode cases"""
    c = fr.case("csa_train", 36, 100)
    other = fr.reference(c, True, seeds=fr.step_seeds(fr.STEP_SEED + 1))
    r = fr.ratios(other, _reference("csa_train", 36, 100, True))
    assert min(r.values()) > 1e-3, r
    r = fr.ratios(_reference("csa_train", 36, 100, False), _reference("csa_train", 36, 100, True))
    assert min(r.values()) > 1e-3, r


@pytest.mark.parametrize("T,N", fr.SMALL + (fr.BIG,), ids=lambda v: str(v))
def test_self_plan_is_the_oracles_block_diagonal_attention(T, N):
    c = fr.case("self", T, N)
    ref = _reference("self", T, N, False)
    p = {f"attention.{n}.weight": w.double() for n, w in c["w"].items()}
    p["attention.norm.weight"] = torch.ones(fr.C, dtype=torch.float64)
    p["attention.norm.bias"] = torch.zeros(fr.C, dtype=torch.float64)
    x = c["x_all"].double()
    y = orc.mha_blockdiag(x, x, x, p, 1, block=T, n_blocks=None)           # (S, N, C)
    err = (ref["xhat"] - y.permute(0, 2, 1)).abs().max().item() / y.abs().max().item()
    print(f"[plan-ref] self T={T} N={N}: {err:.2e} from orc.mha_blockdiag")
    assert err <= 1e-12
