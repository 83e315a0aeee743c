"""CPU-side checks (no GPU needed) of the score-free backward of the cross-length / ragged attention (include/csn_hip.h (3d)):
where csn_cross_attn_flash_available says the flow exists, what the two new entry points refuse on the host, that they leave
the math mode alone, and the host logic of the tuning switches that select the flow."""
import pytest

ARG, ALIGN, DIM = -1, -2, -5


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    L.lib().csn_set_thread_math_mode(-1)
    L.lib().csn_set_math_mode(1)


def _modes(lib):
    """(process mode, per thread?) settings and the state each must leave behind"""
    for mode in (0, 1, 2, 3):
        for per_thread in (False, True):
            if per_thread:
                assert lib.csn_set_math_mode(1 if mode == 0 else 0) == 0          # (the override, not the process mode, decides)
                assert lib.csn_set_thread_math_mode(mode) == 0
            else:
                assert lib.csn_set_thread_math_mode(-1) == 0
                assert lib.csn_set_math_mode(mode) == 0
            yield mode, (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode())


def test_availability_by_math_mode_and_head_width(L):
    lib = L.lib()
    for mode, state in _modes(lib):
        for d in (32, 64, 96, 128):
            assert lib.csn_cross_attn_flash_available(d) == (0 if mode == 0 else 1), (mode, d)
        for d in (256, 40, 0, -32, 16, 160):
            assert lib.csn_cross_attn_flash_available(d) == 0, (mode, d)
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state


def _calls(lib):
    """the two entry points as functions of keyword overrides; pointers are fake, 16-byte aligned and never dereferenced: every
    call below is refused on the host"""
    P = 0x1000
    base = dict(dctx=P, ctx=P, q=P, k=P, v=P, lse=P, delta=P, dq=P, dk=P, dv=P, nq=8, nk=5, d=64, ld_q=8, ld_kv=8, Tp=8, p=0.0,
                nq_arr=P, nk_arr=P)

    def cross(**kw):
        a = dict(base, **kw)
        return lib.csn_cross_attn_bwd_flash_f32(a["dctx"], a["ctx"], 128 * 8, a["q"], a["k"], a["v"], 128 * 8, 128 * 8, a["ld_q"],
                                                a["ld_kv"], a["lse"], a["delta"], a["dq"], a["dk"], a["dv"], 128 * 8, 128 * 8, 1, 2,
                                                a["d"], a["nq"], a["nk"], a["Tp"], a["p"], 1, None)

    def varlen(**kw):
        a = dict(base, **kw)
        return lib.csn_varlen_attn_bwd_flash_f32(a["dctx"], a["ctx"], 128 * 8, a["q"], a["k"], a["v"], 128 * 8, 128 * 8, a["ld_q"],
                                                 a["ld_kv"], a["lse"], a["delta"], a["dq"], a["dk"], a["dv"], 128 * 8, 128 * 8, 1, 2,
                                                 a["d"], a["nq"], a["nk"], a["nq_arr"], a["nk_arr"], a["Tp"], a["p"], 1, None)

    return cross, varlen


def test_new_calls_refuse_bad_arguments_on_the_host(L):
    lib = L.lib()
    cross, varlen = _calls(lib)
    for mode, state in _modes(lib):
        for call in (cross, varlen):
            for name in ("dctx", "ctx", "q", "k", "v", "lse", "delta", "dq", "dk", "dv"):
                assert call(**{name: None}) == ARG, (mode, name)
            assert call(nq=6) == ALIGN and call(nq=0) == ARG and call(nk=0) == ARG
            if mode == 0:
                assert call() == ARG                                           # no score-free flow in exact fp32 ...
                assert call(d=256) == ARG
            else:
                assert call(d=256) == ARG                                      # ... nor at d_head = 256
                assert call(d=40) == DIM
                assert call(p=1.0) == ARG and call(p=-0.1) == ARG
                assert call(ld_q=4) == ARG and call(ld_kv=4) == ARG            # a count beyond its row
                assert call(Tp=4) == ALIGN and call(Tp=10) == ALIGN            # the mask pitch: % 4, >= round-up-4(n_keys)
                assert call(ld_kv=10) == ALIGN
                assert call(q=0x1004) == -3 and call(dk=0x1008) == -3
            assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state, "a refused call changed the math mode"
        assert varlen(nq_arr=None) == ARG and varlen(nk_arr=None) == ARG
        assert (lib.csn_get_math_mode(), lib.csn_get_thread_math_mode()) == state


def test_tuning_switches_are_accepted():
    from csn_amd import tuning
    t = tuning.current()
    assert t.cross_score_free is None and t.cross_score_budget is None         # the kept flow stays the default
    with tuning.override(cross_score_free=True, cross_score_budget=1) as o:
        assert o.cross_score_free is True and o.cross_score_budget == 1 and tuning.current() is o
    with tuning.override(cross_score_free=False):
        assert tuning.current().cross_score_free is False
    assert tuning.current().cross_score_free is None and tuning.current().cross_score_budget is None
    with pytest.raises(TypeError):
        with tuning.override(cross_score_fre=True):
            pass


def test_automatic_rule_is_a_pure_host_function():
    from csn_amd.tuning import cross_takes_score_free as rule
    one = 2 * 4 * 6000 * 6016 * 4
    assert rule(3 * one, 3 * one - 1, True) is True
    assert rule(3 * one, 3 * one, True) is False                               # what fits keeps its flow
    assert rule(3 * one, 288 * 10 ** 9, True) is False
    assert rule(3 * one, 1, True) is True
    assert rule(3 * one, 1, False) is False                                    # never where the kernels have no instance
    assert rule(0, 0, True) is False
    assert rule(387 * 10 ** 9, 288 * 10 ** 9, True) is True
