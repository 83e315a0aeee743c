"""Restatement, with autograd, of the Res16UNet family on voxel rows (csn_amd/minkowski_unet.py), from the pieces of
tests/sparse_conv_ref.py (``Geometry``: the kernel-3 / kernel-5 convolutions) and tests/octant_ref.py (``Partition``: the kernel-2
stride-2 convolution and its transposed form), written out from MinkowskiNet/models/res16unet.py:24-229, resnet.py:86-127 and
modules/resnet_block.py:22-57:

  ``Pyramid``      five coordinate lists at tensor strides 1 .. 16 with their dictionary geometries and partitions
  ``network``      the forward; parameters under ``Res16UNetBase``'s state-dict names; every ReLU optionally a multiplication by a
                   given 0/1 mask.  The graph takes the dtype and device of its inputs: float64 on the CPU is the reference, the
                   same graph in float32 on the device the yardstick of tests/test_gpu_unet.py.  The concatenations are formed.
  ``param_shapes`` / ``params``   names, shapes and fixed random values of a class's parameters and buffers
  ``me_keys``      this project's state-dict names in the reference's layout (``.bn`` under a MinkowskiBatchNorm, ``final.kernel``)"""
import functools

import torch
import torch.nn.functional as F

from tests import octant_ref as O
from tests import sparse_conv_ref as R

EPS, MOMENTUM = 1e-5, 0.02
INIT_DIM = 32
# PLANES and LAYERS of res16unet.py:233-330, the classes csn_amd builds
NETS = {"Res16UNet14": ((32, 64, 128, 256, 256, 256, 256, 256), (1,) * 8),
        "Res16UNet14A": ((32, 64, 128, 256, 128, 128, 96, 96), (1,) * 8),
        "Res16UNet34C": ((32, 64, 128, 256, 256, 128, 96, 96), (2, 3, 4, 6, 2, 2, 2, 2))}
DOWN = ((1, 1), (2, 2), (3, 4), (4, 8))                # convNp{ts}s2
UP = ((4, 16), (5, 8), (6, 4), (7, 2))                 # convtrNp{ts}s2


class Pyramid:
    def __init__(self, coords, stem_kernel=5):
        self.coords = [[tuple(int(v) for v in c) for c in coords]]
        self.s1, self.part = [], []
        for l in range(5):
            ts = 1 << l
            self.s1.append(R.geometry("s1", self.coords[l], k=3, ts=ts)[0])
            if l < 4:
                self.part.append(O.Partition(self.coords[l], ts))
                self.coords.append(self.part[-1].coarse)
        self.stem = R.geometry("s1", self.coords[0], k=stem_kernel, ts=1)[0]
        self._idx = {}

    def octant_rows(self, l, device):
        """Per octant k of the partition of level l: (fine rows, their parents) as index tensors on ``device``."""
        key = (l, str(device))
        if key not in self._idx:
            p = self.part[l]
            out = []
            for k in range(8):
                rows = [i for i in range(p.n_fine) if p.octant[i] == k]
                out.append((torch.tensor(rows, dtype=torch.long, device=device),
                            torch.tensor([p.parent[i] for i in rows], dtype=torch.long, device=device)))
            self._idx[key] = out
        return self._idx[key]


def conv(g, x, w):
    y = x.new_zeros(g.n_out, w.shape[2])
    for kidx, (j, i) in enumerate(g.pairs):
        if len(j):
            y = y.index_add(0, j.to(x.device), x[i.to(x.device)] @ w[kidx])
    return y


def octant_down(pyr, l, x, w):
    y = x.new_zeros(pyr.part[l].n_coarse, w.shape[2])
    for k, (rows, par) in enumerate(pyr.octant_rows(l, x.device)):
        if len(rows):
            y = y.index_add(0, par, x[rows] @ w[k])
    return y


def octant_up(pyr, l, x, w):
    y = x.new_zeros(pyr.part[l].n_fine, w.shape[2])
    for k, (rows, par) in enumerate(pyr.octant_rows(l, x.device)):
        if len(rows):
            y = y.index_add(0, rows, x[par] @ w[k])
    return y


def network(pyr, feats, p, net, training, masks=None, eps=EPS, momentum=MOMENTUM):
    """Returns (logits, pre: name -> pre-activation of every ReLU (the keys of the model's trace), new: name -> (running_mean,
    running_var) after this batch)."""
    planes, layers = NETS[net]
    pre, new = {}, {}

    def bn(z, name):
        rm, rv = p[name + ".running_mean"].clone(), p[name + ".running_var"].clone()
        y = F.batch_norm(z, rm, rv, p[name + ".weight"], p[name + ".bias"], training, momentum, eps)
        new[name] = (rm, rv)
        return y

    def act(name, a):
        pre[name] = a
        return a.clamp_min(0) if masks is None else a * masks[name].to(a.dtype).to(a.device)

    def blocks(name, x, l, n):
        for i in range(n):
            q = f"{name}.{i}."
            h = act(q + "norm1", bn(conv(pyr.s1[l], x, p[q + "conv1.kernel"]), q + "norm1"))
            a = bn(conv(pyr.s1[l], h, p[q + "conv2.kernel"]), q + "norm2")
            r = bn(x @ p[q + "downsample.0.kernel"][0], q + "downsample.1") if q + "downsample.0.kernel" in p else x
            x = act(q + "norm2", a + r)
        return x

    out_p1 = act("bn0", bn(conv(pyr.stem, feats, p["conv0p1s1.kernel"]), "bn0"))
    skips, out = [out_p1], out_p1
    for n, ts in DOWN:
        out = act(f"bn{n}", bn(octant_down(pyr, n - 1, out, p[f"conv{n}p{ts}s2.kernel"]), f"bn{n}"))
        out = blocks(f"block{n}", out, n, layers[n - 1])
        skips.append(out)
    skips.pop()
    for n, ts in UP:
        l = 7 - n
        out = act(f"bntr{n}", bn(octant_up(pyr, l, out, p[f"convtr{n}p{ts}s2.kernel"]), f"bntr{n}"))
        out = blocks(f"block{n + 1}", torch.cat([out, skips.pop()], dim=1), l, layers[n])
    return out @ p["final.weight"].t() + p["final.bias"], pre, new


def param_shapes(net, in_channels=3, out_channels=6, stem_kernel=5):
    """name -> shape of every parameter and buffer, under this project's names."""
    planes, layers = NETS[net]
    out = {}

    def norm(name, c):
        for q in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.{q}"] = (c,)
        out[f"{name}.num_batches_tracked"] = ()

    def layer(name, inplanes, c, n):
        for i in range(n):
            ci = inplanes if i == 0 else c
            out[f"{name}.{i}.conv1.kernel"] = (27, ci, c)
            norm(f"{name}.{i}.norm1", c)
            out[f"{name}.{i}.conv2.kernel"] = (27, c, c)
            norm(f"{name}.{i}.norm2", c)
            if ci != c:
                out[f"{name}.{i}.downsample.0.kernel"] = (1, ci, c)
                norm(f"{name}.{i}.downsample.1", c)

    inplanes = INIT_DIM
    out["conv0p1s1.kernel"] = (stem_kernel ** 3, in_channels, inplanes)
    norm("bn0", inplanes)
    for n, ts in DOWN:
        out[f"conv{n}p{ts}s2.kernel"] = (8, inplanes, inplanes)
        norm(f"bn{n}", inplanes)
        layer(f"block{n}", inplanes, planes[n - 1], layers[n - 1])
        inplanes = planes[n - 1]
    skips = (planes[2], planes[1], planes[0], INIT_DIM)
    for n, ts in UP:
        out[f"convtr{n}p{ts}s2.kernel"] = (8, inplanes, planes[n])
        norm(f"bntr{n}", planes[n])
        layer(f"block{n + 1}", planes[n] + skips[n - 4], planes[n], layers[n])
        inplanes = planes[n]
    out["final.weight"] = (out_channels, planes[7])
    out["final.bias"] = (out_channels,)
    return out


@functools.lru_cache(maxsize=None)
def params(net, seed=0):
    """float32 CPU parameters (never modified): kernels of variance 1 / (KV c_in), BatchNorm weights near 1, running statistics near
    (0, 1)."""
    g = torch.Generator().manual_seed(2000 + seed + len(net))
    r = lambda *s: torch.randn(*s, generator=g)
    p = {}
    for name, shape in param_shapes(net).items():
        if name.endswith(".kernel"):
            p[name] = r(*shape) / (shape[0] * shape[1]) ** 0.5
        elif name == "final.weight":
            p[name] = r(*shape) / shape[1] ** 0.5
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


def me_keys(names):
    """This project's state-dict names -> the reference's: a MinkowskiBatchNorm wraps its norm (``.bn``), ``final`` is a convolution."""
    out = []
    for n in names:
        head, leaf = n.rsplit(".", 1)
        if n == "final.weight":
            out.append("final.kernel")
        elif leaf != "kernel" and head != "final":
            out.append(f"{head}.bn.{leaf}")
        else:
            out.append(n)
    return out
