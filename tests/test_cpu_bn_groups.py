"""CPU-side checks of BatchNorm over row groups (include/csn_hip.h section 20): the float64 statement tests/bn_groups_ref.py pinned
against ``torch.nn.functional.batch_norm`` applied per group in float64 (outputs and, through autograd, every gradient, to 1e-12);
``merge_batches`` on the torch backend on CPU tensors; the new symbols in the header, the library and the binding; the tuning switch's
default; CPU rows refused."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import bn_groups_ref as G
from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csn_sparse_conv_stats_groups_workspace_bytes", "csn_sparse_conv_stats_groups_fwd_f32", "csn_rows_bn_act_groups_workspace_bytes",
       "csn_rows_bn_act_groups_fwd_f32", "csn_rows_bn_act_groups_bwd_f32")


def _case(M, n, C, seed=0):
    g = torch.Generator().manual_seed(1 + seed + 7 * M + n + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    terms = [{"z": ((0.5 + m) * r(n, C) + 0.3 * m).requires_grad_(True), "gamma": (1 + 0.2 * r(C)).requires_grad_(True),
              "beta": (0.3 * r(C)).requires_grad_(True)} for m in range(M)]
    return terms, r(n, C).requires_grad_(True), r(n, C)


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (True, False)])
def test_statement_equals_batch_norm_per_group(M, res, relu):
    off = G.layout(260)
    terms, r, dy = _case(M, 260, 32)
    y, _ = G.bn_act_groups(terms, off, r if res else None, relu)
    a = 0
    for t in terms:
        a = a + torch.cat([F.batch_norm(t["z"][lo:hi], None, None, t["gamma"], t["beta"], True, 0.0, G.EPS) for lo, hi in zip(off, off[1:])])
    if res:
        a = a + r
    want = a.clamp_min(0) if relu else a
    assert (y - want).abs().max() < 1e-12
    leaves = [v for t in terms for v in (t["z"], t["gamma"], t["beta"])] + ([r] if res else [])
    got, ref = torch.autograd.grad(y, leaves, dy), torch.autograd.grad(want, leaves, dy)
    for a, b in zip(got, ref):
        assert (a - b).abs().max() <= 1e-12 * max(1.0, b.abs().max().item())


def test_running_statistics_recursion_is_sequential_batch_norm():
    off = G.layout(300)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(300, 32, generator=g, dtype=torch.float64) * 2 + 1
    rm, rv = 0.1 * torch.randn(32, generator=g, dtype=torch.float64), 1 + torch.rand(32, generator=g, dtype=torch.float64)
    got = G.stats_groups(z, off, G.EPS, 0.1, rm, rv)
    a, b = rm.clone(), rv.clone()
    for i, (lo, hi) in enumerate(zip(off, off[1:])):
        F.batch_norm(z[lo:hi], a, b, None, None, True, 0.1, G.EPS)
        one = H.stats(z[lo:hi], G.EPS)
        assert (got["mean"][i] - one["mean"]).abs().max() < 1e-12 and (got["invstd"][i] - one["invstd"]).abs().max() < 1e-12
    assert (got["running_mean"] - a).abs().max() < 1e-12 and (got["running_var"] - b).abs().max() < 1e-12


def test_backbone_groups_sums_weight_gradients_and_hands_on_running_statistics():
    sets = [G.sorted_set(31), G.sorted_set(33)]
    pyrs = [H.Pyramid(s, 2) for s in sets]
    g = torch.Generator().manual_seed(9)
    feats = [torch.randn(len(s), 3, generator=g, dtype=torch.float64) for s in sets]
    p = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in H.params(2, 4).items()}
    rows, _, new = G.backbone_groups(pyrs, feats, p, 2, True)
    w = p["conv0s1.kernel"]
    total, = torch.autograd.grad(sum(r.sum() for r in rows), [w])
    # group by group by hand: the second group sees the first one's running statistics; the weight gradient is the groups' sum
    y0, _, n0 = H.backbone(pyrs[0], feats[0], p, 2, True)
    p1 = dict(p)
    for name, (rm, rv) in n0.items():
        p1[name + ".running_mean"], p1[name + ".running_var"] = rm, rv
    y1, _, n1 = H.backbone(pyrs[1], feats[1], p1, 2, True)
    g0, = torch.autograd.grad(y0.sum(), [w])
    g1, = torch.autograd.grad(y1.sum(), [w])
    assert (total - (g0 + g1)).abs().max() <= 1e-12 * total.abs().max()
    assert torch.equal(new["bn0s1"][0], n1["bn0s1"][0]) and not torch.equal(n0["bn0s1"][0], n1["bn0s1"][0])


# ------------------------------------------------------------------------------------------------------
# merge_batches
# ------------------------------------------------------------------------------------------------------
def _shift(t, a):
    return torch.where(t >= 0, t + a, t)


@pytest.mark.parametrize("given", [False, True], ids=["derived", "n_shapes"])
def test_merge_batches_equals_the_separate_pyramids_with_row_offsets_added(given):
    from csn_amd import build_pyramid, merge_batches
    sets = [torch.tensor(G.sorted_set(n)) for n in (31, 33, 129)]
    gp = merge_batches([(c, None) for c in sets], 3, n_shapes=[2, 2, 2] if given else None, backend="torch")
    assert gp.n_groups == 3 and gp.n_shapes == [2, 2, 2] and gp.shape_offsets == [0, 2, 4, 6]
    assert gp.n_levels == 3 and gp.stem_kernel == 5
    own = [build_pyramid(c, 3, backend="torch") for c in sets]
    for l in range(3):
        off = gp.group_rows_host[l]
        assert off[0] == 0 and off[-1] == gp.coords[l].shape[0]
        assert gp.group_rows[l].dtype == torch.int32 and gp.group_rows[l].tolist() == off
        for g, p in enumerate(own):
            a, b = off[g], off[g + 1]
            assert b - a == p.coords[l].shape[0]
            want = p.coords[l].clone()
            want[:, 0] += 2 * g
            assert torch.equal(gp.coords[l][a:b], want)                     # the same rows in the same order
            assert torch.equal(gp.s1[l].fwd[:, a:b], _shift(p.s1[l].fwd, a))
            if l == 0:
                assert torch.equal(gp.stem.fwd[:, a:b], _shift(p.stem.fwd, a))
            if l + 1 < 3:
                a2, b2 = gp.group_rows_host[l + 1][g], gp.group_rows_host[l + 1][g + 1]
                assert torch.equal(gp.down[l].fwd[:, a2:b2], _shift(p.down[l].fwd, a))          # indexed by coarse rows, holds fine rows
                assert torch.equal(gp.down[l].bwd_table[:, a:b], _shift(p.down[l].bwd_table, a2))
                assert torch.equal(gp.up(l).fwd[:, a:b], _shift(p.up(l).fwd, a2))
    # the shape offsets the head needs: every group's own, from 0
    from csn_amd.minkowski_csn import offsets_from_batch_index
    for g, c in enumerate(sets):
        assert gp.group_offsets(g) == offsets_from_batch_index(c[:, 0]).tolist()


def test_merge_batches_refusals():
    from csn_amd import merge_batches
    a = torch.tensor(G.sorted_set(31))
    one = torch.tensor([[0, 5, 5, 5]])
    with pytest.raises(ValueError, match="more than 1 value"):             # a one-row group, in conv_stats' wording
        merge_batches([(a, None), (one, None)], 1, backend="torch")
    lonely = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]])                     # two rows at level 0, ONE at level 1
    with pytest.raises(ValueError, match="more than 1 value"):
        merge_batches([(a, None), (lonely, None)], 2, backend="torch")
    with pytest.raises(ValueError, match="8"):
        merge_batches([(a, None)] * 9, 1, backend="torch")
    with pytest.raises(ValueError):
        merge_batches([], 1, backend="torch")
    with pytest.raises(ValueError, match="sorted"):
        merge_batches([(torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [1, 3, 0, 0]]), None)], 1, n_shapes=[2], backend="torch")
    far = a.clone()
    far[:, 0] += (1 << 15) - 3                                              # shifted batch indices leave build_pyramid's range
    with pytest.raises(ValueError):
        merge_batches([(far, None), (a, None)], 1, backend="torch")


# ------------------------------------------------------------------------------------------------------
# ABI, switch, refusals
# ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_binding():
    from csn_amd import _lib
    _lib.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(csn_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (csn_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert name in declared and name in exported and name in _lib.EXPORTS, name
    assert _lib.lib().csn_version() == 17
    assert "#define CSN_ABI_VERSION 17" in open(os.path.join(ROOT, "include", "csn_hip.h")).read()


def test_bad_arguments_are_refused_on_the_host():
    from csn_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert lib.csn_rows_bn_act_groups_workspace_bytes(260, 32, 1, 0) == 0 and lib.csn_rows_bn_act_groups_workspace_bytes(260, 32, 1, 9) == 0
    assert lib.csn_rows_bn_act_groups_workspace_bytes(260, 48, 1, 2) == 0
    one = lib.csn_rows_bn_act_workspace_bytes(260, 32, 2)
    assert lib.csn_rows_bn_act_groups_workspace_bytes(260, 32, 2, 1) == one              # one group: no part more than (15b)
    assert lib.csn_rows_bn_act_groups_workspace_bytes(260, 32, 2, 6) > one
    assert lib.csn_sparse_conv_stats_groups_workspace_bytes(260, 32, 9) == 0
    assert lib.csn_sparse_conv_stats_groups_workspace_bytes(260, 32, 6) == lib.csn_sparse_conv_stats_workspace_bytes(260, 32)
    t = _lib.BnTerms()
    import ctypes
    assert lib.csn_rows_bn_act_groups_fwd_f32(ctypes.addressof(t), 1, 260, 32, None, 2, None, 0, 1, None, 32, None) == -1
    assert lib.csn_rows_bn_act_groups_bwd_f32(None, 32, None, 32, ctypes.addressof(t), 1, 260, 32, None, 2, 1, None, 32, None, 0, None) == -1
    assert lib.csn_sparse_conv_stats_groups_fwd_f32(None, 32, 260, None, 260, 27, 32, 32, None, None, 32, None, None, None, None, 1e-5, 0.1,
                                                    None, 2, None, 0, None) == -1


def test_switch_is_off_by_default():
    from csn_amd import tuning
    assert tuning.current().grouped_passes is False
    with tuning.override(grouped_passes=True) as t:
        assert t.grouped_passes is True
    assert tuning.current().grouped_passes is False


def test_cpu_rows_are_refused():
    from csn_amd import CsnError, HRNetBackbone, bn_act_groups, conv_stats_groups, merge_batches
    from csn_amd.minkowski_conv import build_kernel_map
    pts = torch.tensor(G.sorted_set(31))
    m = build_kernel_map(pts)
    off = torch.tensor([0, 10, 31], dtype=torch.int32)
    x, w = torch.zeros(31, 32), torch.zeros(27, 32, 32)
    with pytest.raises(CsnError):
        conv_stats_groups(x, w, m, off, None, None, 1e-5, 0.02)
    v = torch.zeros(2, 32)
    with pytest.raises(CsnError):
        bn_act_groups([(x, v, v, torch.ones(32), torch.zeros(32))], off)
    gp = merge_batches([(pts, None), (pts, None)], 2, backend="torch")
    with pytest.raises(CsnError):
        HRNetBackbone(3, 2, 4)(torch.zeros(62, 3), gp)
