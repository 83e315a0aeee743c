"""float64 restatement, with autograd, of the HRNet backbone on voxel rows (csn_amd/minkowski_hrnet.py, include/csn_hip.h section
15), built on tests/sparse_conv_ref.py's ``Geometry``:

  ``stats``      (15a) mean, invstd and the running-statistics update of a map's BatchNorm batch
  ``bn_act``     (15b) y = act(sum_m batch_norm(z_m) + r): autograd through ``F.batch_norm`` is the complete BatchNorm gradient
  ``R.block``    the block (tests/sparse_conv_ref.py)
  ``backbone``   ``forward_backbone`` + final transitions + concatenation (MinkowskiNet/models/hrnet.py:122-163, 308-326, 433-437),
                 parameters named as ``HRNetBackbone``'s state dict; every ReLU is optionally a multiplication by a given 0/1 mask.
tests/test_cpu_hrnet.py pins ``backbone`` to the same network written with torch's dense convolutions."""
import functools

import torch
import torch.nn.functional as F

from tests import sparse_conv_ref as R

EPS, MOMENTUM = 1e-5, 0.02


def stats(z, eps=EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    z = z.double()
    n = z.shape[0]
    mean, var = z.mean(0), z.var(0, unbiased=False)
    out = {"mean": mean, "invstd": (var + eps).rsqrt()}
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * running_mean.double() + momentum * mean
    if running_var is not None:
        out["running_var"] = (1 - momentum) * running_var.double() + momentum * var * n / (n - 1)
    return out


def bn_act(terms, r, relu, training, eps=EPS, mask=None):
    """terms: dicts z, gamma, beta and (eval) running_mean, running_var — float64, requires_grad where a gradient is wanted.
    Returns (y, pre-activation)."""
    a = 0
    for t in terms:
        rm = None if training else t["running_mean"]
        rv = None if training else t["running_var"]
        a = a + F.batch_norm(t["z"], rm, rv, t["gamma"], t["beta"], training, 0.0, eps)
    if r is not None:
        a = a + r
    if not relu:
        return a, a
    return (a.clamp_min(0) if mask is None else a * mask.double()), a


class Pyramid:
    """Coordinate lists and dictionary geometries of ``n_levels`` levels: s1[l], stem, down[l] (l -> l + 1), up[l] (l + 1 -> l)."""

    def __init__(self, coords, n_levels, stem_kernel=5):
        self.coords = [[tuple(int(v) for v in c) for c in coords]]
        self.s1, self.down, self.up = [], [], []
        for l in range(n_levels):
            ts = 1 << l
            self.s1.append(R.geometry("s1", self.coords[l], k=3, ts=ts)[0])
            if l + 1 < n_levels:
                g, out = R.geometry("s2", self.coords[l], ts=ts)
                self.down.append(g)
                self.coords.append(out)
                self.up.append(R.geometry("tr", out, ts=ts, fine=self.coords[l])[0])
        self.stem = R.geometry("s1", self.coords[0], k=stem_kernel, ts=1)[0]


def conv(g, x, w):
    return R._conv_autograd(g, x, w)


def backbone(pyr, feats, p, num_stages, training, masks=None, eps=EPS, momentum=MOMENTUM, conv_fn=conv):
    """Returns (rows (N, init_dim + branch widths), pre: name -> pre-activation of every ReLU (the keys of ``HRNetBackbone``'s
    trace), new: name -> (running_mean, running_var) after this batch).  ``p``: float64 tensors under ``HRNetBackbone``'s state-dict
    names.  ``conv_fn(geometry, x, w)`` is the convolution (the dense pin swaps it)."""
    pre, new = {}, {}

    def bn(z, name):
        rm, rv = p[name + ".running_mean"].clone(), p[name + ".running_var"].clone()
        y = F.batch_norm(z, rm, rv, p[name + ".weight"], p[name + ".bias"], training, momentum, eps)
        new[name] = (rm, rv)
        return y

    def act(name, a):
        pre[name] = a
        return a.clamp_min(0) if masks is None else a * masks[name].double()

    def cb(cname, nname, x, g):
        return bn(conv_fn(g, x, p[cname + ".kernel"]), nname)

    out_init = act("bn0s1", cb("conv0s1", "bn0s1", feats, pyr.stem))
    out = act("bn1s1", cb("conv1s1", "bn1s1", out_init, pyr.s1[0]))
    stage_input = [out]
    for i in range(num_stages):
        stage_output = []
        for j in range(i + 1):
            x = stage_input[j]
            for b in range(3):
                n = f"stages.{i}.{j}.{b}."
                h = act(n + "norm1", cb(n + "conv1", n + "norm1", x, pyr.s1[j]))
                x = act(n + "norm2", cb(n + "conv2", n + "norm2", h, pyr.s1[j]) + x)
            stage_output.append(x)
        if i == num_stages - 1:
            break
        depth = i + 1
        stage_input = []
        for k in range(depth + 1):
            buf = None
            for j in range(depth):
                if j == k:
                    t = stage_output[j]
                else:
                    t, steps = stage_output[j], abs(k - j)
                    for s in range(steps):
                        g = pyr.down[j + s] if k > j else pyr.up[j - s - 1]
                        n = f"exchange_blocks.{i}.{j}.{k}."
                        t = cb(n + str(3 * s), n + str(3 * s + 1), t, g)
                        if s + 1 < steps:
                            t = act(n + str(3 * s + 1), t)
                buf = t if buf is None else buf + t
            stage_input.append(act(f"sum.{i}.{k}", buf))
    outs = [out_init, stage_output[0]]
    for i in range(1, num_stages):
        x = stage_output[i]
        for s in range(i):
            n = f"final_transitions.{i - 1}."
            x = act(n + str(3 * s + 1), cb(n + str(3 * s), n + str(3 * s + 1), x, pyr.up[i - s - 1]))
        outs.append(x)
    return torch.cat(outs, dim=1), pre, new


def param_shapes(num_stages, feat_factor, in_channels=3, init_dim=32, stem_kernel=5):
    """name -> shape of every parameter and buffer of the backbone, written out from hrnet.py's constructor (:31-120, 308-326) and
    resnet_block.py:22-39, under this project's names (the MinkowskiBatchNorm wrapper's ``.bn`` level dropped)."""
    D = init_dim * feat_factor
    out = {}

    def norm(name, c):
        for q in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.{q}"] = (c,)
        out[f"{name}.num_batches_tracked"] = ()

    out["conv0s1.kernel"] = (stem_kernel ** 3, in_channels, init_dim)
    norm("bn0s1", init_dim)
    out["conv1s1.kernel"] = (27, init_dim, D)
    norm("bn1s1", D)
    for i in range(num_stages):
        for j in range(i + 1):
            c = D * 2 ** j
            for b in range(3):
                for q in ("1", "2"):
                    out[f"stages.{i}.{j}.{b}.conv{q}.kernel"] = (27, c, c)
                    norm(f"stages.{i}.{j}.{b}.norm{q}", c)
        if i == num_stages - 1:
            break
        depth = i + 1
        for j in range(depth):
            c0 = D * 2 ** j
            for k in range(depth + 1):
                idx = 0
                for s in range(abs(k - j)):
                    if s:
                        idx += 1                                           # the ReLU between two steps
                    ci, co = (c0 * 2 ** s, c0 * 2 ** (s + 1)) if k > j else (c0 // 2 ** s, c0 // 2 ** (s + 1))
                    out[f"exchange_blocks.{i}.{j}.{k}.{idx}.kernel"] = (27, ci, co)
                    norm(f"exchange_blocks.{i}.{j}.{k}.{idx + 1}", co)
                    idx += 2
    for i in range(1, num_stages):
        c = D * 2 ** i
        for s in range(i):
            out[f"final_transitions.{i - 1}.{3 * s}.kernel"] = (27, c, c)
            norm(f"final_transitions.{i - 1}.{3 * s + 1}", c)
    return out


@functools.lru_cache(maxsize=None)
def params(num_stages, feat_factor, seed=0, in_channels=3):
    """float32 CPU parameters of a backbone (never modified): kernels of variance 1 / (KV c_in), BatchNorm weights near 1, running
    statistics near (0, 1)."""
    g = torch.Generator().manual_seed(1000 + seed + 10 * num_stages)
    r = lambda *s: torch.randn(*s, generator=g)
    p = {}
    for name, shape in param_shapes(num_stages, feat_factor, in_channels).items():
        if name.endswith(".kernel"):
            p[name] = r(*shape) / (shape[0] * shape[1]) ** 0.5
        elif name.endswith(".weight"):
            p[name] = 1 + 0.2 * r(*shape)
        elif name.endswith(".bias"):
            p[name] = 0.3 * r(*shape)
        elif name.endswith(".running_mean"):
            p[name] = 0.1 * r(*shape)
        elif name.endswith(".running_var"):
            p[name] = 1 + 0.1 * r(*shape).abs()
        else:
            p[name] = torch.zeros((), dtype=torch.long)
    return p


def two_coarse_rows(n_levels):
    """A point set whose level ``n_levels - 1`` has exactly 2 rows: two shapes, each a partly filled cube of side 2^(n_levels - 1)
    anchored at a multiple of that side (negative for shape 1)."""
    side = 1 << (n_levels - 1)
    pts = []
    for b, base in ((0, 0), (1, -side)):
        for z in range(side):
            for y in range(side):
                for x in range(side):
                    if (x + 2 * y + 3 * z + b) % 3 != 1:
                        pts.append([b, base + x, y, base + z])
    return pts
