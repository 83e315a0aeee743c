"""float64 statement of BatchNorm over row groups (include/csn_hip.h section 20; csn_amd.minkowski_hrnet.conv_stats_groups /
bn_act_groups / merge_batches), on tests/hrnet_ref.py and tests/sparse_conv_ref.py:

  ``stats_groups``     (20a) per group g = rows [group_rows[g], group_rows[g + 1]): mean, invstd, and the running statistics after the
                       G updates in group order 0 .. G - 1, each with that group's mean and its n / (n - 1) variance
  ``bn_act_groups``    (20b) y_i = act(sum_m (gamma_m (z_m,i - mu_m[g]) s_m[g] + beta_m) + r_i), the statistics written out from the
                       group's own rows (no ``F.batch_norm``: tests/test_cpu_bn_groups.py pins this to it); autograd through the
                       statistics is the complete BatchNorm gradient per group, dgamma / dbeta over all rows
  ``conv_bn_act_groups``  convolution + per-group BatchNorm + sum + ReLU
  ``backbone_groups``  a whole backbone evaluated GROUP BY GROUP on ``hrnet_ref.backbone`` — every group its own pyramid and BatchNorm
                       batch, the running statistics handed from group to group; the parameters are shared leaves, so autograd sums
                       the weight gradients over the groups
"""
import torch

from tests import hrnet_ref as H
from tests import sparse_conv_ref as R

EPS, MOMENTUM = H.EPS, H.MOMENTUM
# (20a) / (20b) group layouts: every boundary case of the 32-row statistics tile, the 64-row chunk and the 128-row work-group tile —
# 5: inside a tile; 5 + 27 = 32: on a tile edge; + 33 = 65: inside the second chunk; + 63 = 128: on a work-group tile's edge;
# + 129 = 257 and + 3 = 260: two boundaries inside one tile (a group of fewer than 32 rows); the last group ends in a partial tile
COUNTS = (5, 27, 33, 63, 129, 3)


def layout(n):
    """Group row offsets for n rows: ``COUNTS`` (260 rows), and one more group for what is left (at least 3 rows)."""
    assert n == 260 or n >= 263
    counts = list(COUNTS) + ([n - 260] if n > 260 else [])
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def stats_groups(z, group_rows, eps=EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    z = z.double()
    out = {"mean": [], "invstd": []}
    rm = None if running_mean is None else running_mean.double().clone()
    rv = None if running_var is None else running_var.double().clone()
    for a, b in zip(group_rows, group_rows[1:]):
        zg, n = z[a:b], b - a
        mean, var = zg.mean(0), zg.var(0, unbiased=False)
        out["mean"].append(mean)
        out["invstd"].append((var + eps).rsqrt())
        if rm is not None:
            rm = (1 - momentum) * rm + momentum * mean
        if rv is not None:
            rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    out["mean"], out["invstd"] = torch.stack(out["mean"]), torch.stack(out["invstd"])
    if rm is not None:
        out["running_mean"] = rm
    if rv is not None:
        out["running_var"] = rv
    return out


def bn_act_groups(terms, group_rows, r, relu, eps=EPS, mask=None):
    """terms: dicts z, gamma, beta (float64, requires_grad where a gradient is wanted).  Returns (y, pre-activation)."""
    a = 0
    for t in terms:
        parts = []
        for lo, hi in zip(group_rows, group_rows[1:]):
            zg = t["z"][lo:hi]
            mu = zg.mean(0)
            s = ((zg - mu).square().mean(0) + eps).rsqrt()
            parts.append(t["gamma"] * ((zg - mu) * s) + t["beta"])
        a = a + torch.cat(parts)
    if r is not None:
        a = a + r
    if not relu:
        return a, a
    return (a.clamp_min(0) if mask is None else a * mask.double()), a


def conv_bn_act_groups(g, x, w, gamma, beta, group_rows, r=None, relu=True, eps=EPS, mask=None):
    return bn_act_groups([{"z": H.conv(g, x, w), "gamma": gamma, "beta": beta}], group_rows, r, relu, eps, mask)


def backbone_groups(pyrs, feats, p, num_stages, training, masks=None):
    """``hrnet_ref.backbone`` on every group in order; ``masks``: one dict per group or None.  Returns (rows per group, pre per group,
    new: name -> (running_mean, running_var) after the last group)."""
    rows, pres, new = [], [], {}
    cur = dict(p)
    for i, (pyr, f) in enumerate(zip(pyrs, feats)):
        y, pre, new = H.backbone(pyr, f, cur, num_stages, training, masks=None if masks is None else masks[i])
        rows.append(y)
        pres.append(pre)
        cur = dict(cur)
        for name, (rm, rv) in new.items():
            cur[name + ".running_mean"], cur[name + ".running_var"] = rm, rv
    return rows, pres, new


def sorted_set(n, seed=0):
    """``sparse_conv_ref.random_set`` with its rows sorted by shape (any order inside a shape), as a batch must be."""
    return sorted(R.random_set(n, seed=seed), key=lambda c: c[0])
