"""float64 restatement of the sparse 3D convolution on voxel rows (csn_amd/minkowski_conv.py, include/csn_hip.h section 14), written
from the definitions with a coordinate dictionary — no tables:

  offsets o = (ox, oy, oz) in [-r, r]^3, kidx = (ox + r) + k (oy + r) + k^2 (oz + r); weight (KV, c_in, c_out)
  "s1"  stride 1:            out coords = in coords,                                   y[c]  = sum_o x[c  + ts o] W[kidx(o)]
  "s2"  stride 2, k = 3:     out coords = sorted unique [b, floor(xyz / 2ts) 2ts],     y[c'] = sum_o x[c' + ts o] W[kidx(o)]
  "tr"  transposed, k = 3:   from the coarse set onto a given fine set at ts,          y[c]  = sum_o x[c  - ts o] W[kidx(o)]

``Geometry`` lists, per offset, the (output row, input row) pairs the definition names; ``fwd`` and ``bwd`` are sums over those
pairs.  tests/test_cpu_sparse_conv.py pins them to torch's dense conv3d / conv_transpose3d; the GPU tests take them as their
yardstick.  The point sets of the tests live here too, so that both files see the same ones."""
import functools

import numpy as np
import torch


def offsets(k):
    r = k // 2
    return [(ox, oy, oz) for oz in range(-r, r + 1) for oy in range(-r, r + 1) for ox in range(-r, r + 1)]


def down_coords(coords, ts):
    """Sorted unique [b, floor(xyz / 2ts) 2ts] (python's // is floor)."""
    s = 2 * ts
    return sorted({(b, x // s * s, y // s * s, z // s * s) for b, x, y, z in coords})


class Geometry:
    """pairs[kidx] = (out rows j, in rows i) int64 tensors of one convolution between two coordinate lists (of 4-tuples)."""

    def __init__(self, in_coords, out_coords, k, ts, sign):
        self.n_in, self.n_out, self.k, self.KV = len(in_coords), len(out_coords), k, k ** 3
        where = {c: i for i, c in enumerate(in_coords)}
        assert len(where) == len(in_coords)
        self.pairs = []
        for ox, oy, oz in offsets(k):
            js, is_ = [], []
            for j, (b, x, y, z) in enumerate(out_coords):
                i = where.get((b, x + sign * ts * ox, y + sign * ts * oy, z + sign * ts * oz))
                if i is not None:
                    js.append(j)
                    is_.append(i)
            self.pairs.append((torch.tensor(js, dtype=torch.long), torch.tensor(is_, dtype=torch.long)))


def geometry(mode, coords, k=3, ts=1, fine=None):
    """mode "s1" / "s2": ``coords`` are the input set at ts.  mode "tr": ``coords`` are the coarse input set at 2 ts, ``fine`` the
    output set at ts.  Returns (Geometry, out coords as a list of tuples)."""
    coords = [tuple(int(v) for v in c) for c in coords]
    if mode == "s1":
        return Geometry(coords, coords, k, ts, 1), coords
    if mode == "s2":
        out = down_coords(coords, ts)
        return Geometry(coords, out, 3, ts, 1), out
    fine = [tuple(int(v) for v in c) for c in fine]
    return Geometry(coords, fine, 3, ts, -1), fine


def fwd(g, x, w, bias=None):
    x, w = x.double(), w.double()
    y = torch.zeros(g.n_out, w.shape[2], dtype=torch.float64)
    for kidx, (j, i) in enumerate(g.pairs):
        if len(j):
            y.index_add_(0, j, x[i] @ w[kidx])
    return y if bias is None else y + bias.double().reshape(1, -1)


def bwd(g, dy, x, w):
    """dx, dw, dbias of ``fwd`` for the upstream dy, and per tensor the same contraction over absolute values of every term
    (``scale_*``: what a gradient is measured against where the true one nearly cancels)."""
    dy, x, w = dy.double(), x.double(), w.double()
    dx, adx = torch.zeros_like(x), torch.zeros_like(x)
    dw, adw = torch.zeros_like(w), torch.zeros_like(w)
    for kidx, (j, i) in enumerate(g.pairs):
        if len(j):
            dx.index_add_(0, i, dy[j] @ w[kidx].t())
            adx.index_add_(0, i, dy[j].abs() @ w[kidx].abs().t())
            dw[kidx] = x[i].t() @ dy[j]
            adw[kidx] = x[i].abs().t() @ dy[j].abs()
    return {"dx": dx, "dw": dw, "dbias": dy.sum(0), "scale_dx": adx.max(), "scale_dw": adw.max(), "scale_dbias": dy.abs().sum(0).max()}


# ------------------------------------------------------------------------------------------------------
# point sets (lists of [b, x, y, z]; x, y, z multiples of ts; negative coordinates included; rows in random order)
# ------------------------------------------------------------------------------------------------------
def single_voxel(ts=1):
    return [[0, -3 * ts, 2 * ts, 5 * ts]]


def dense_block(ts=1, side=4):
    return [[0, (x - 2) * ts, (y - 1) * ts, z * ts] for z in range(side) for y in range(side) for x in range(side)]


def random_set(n=None, ts=1, seed=0):
    """Occupancy ~0.15 of a cube for 2 shapes with the same xyz range (so shape 0 and shape 1 share many xyz), shuffled and trimmed
    to n rows (None: untrimmed).  The cube is 12^3 (about 518 voxels) up to n = 400, 16^3 (about 1229) up to n = 1100 and 48^3
    (about 33000) beyond it."""
    side = 12 if (n is None or n <= 400) else (16 if n <= 1100 else 48)
    rng = np.random.default_rng(100 + seed + (n or 0))
    rows = [[b, (x - side // 2) * ts, (y - side // 2) * ts, (z - side // 2) * ts]
            for b in range(2) for z in range(side) for y in range(side) for x in range(side) if rng.random() < 0.15]
    rng.shuffle(rows)
    assert n is None or len(rows) >= n
    return rows[:n]


def two_clusters(ts=1, seed=0):
    """Two 5^3 clusters at occupancy 0.7, 2000 voxels apart in one shape, then a line of isolated voxels: the last 128-row tile
    holds isolated voxels only, so it skips every offset but the centre."""
    rng = np.random.default_rng(7 + seed)
    out = []
    for base in (-1000, 1000):
        pts = [[0, (base + x) * ts, y * ts, (z - 2) * ts] for z in range(5) for y in range(5) for x in range(5) if rng.random() < 0.7]
        out += pts
    return out + [[0, 0, 0, 40 * ts * i] for i in range(1, 140)]      # 139 isolated voxels: only the centre offset exists


@functools.lru_cache(maxsize=None)
def tensors(seed, n_in, n_out, KV, c_in, c_out):
    """x, w (variance 1 / (KV c_in): outputs O(1)), bias, dy — float32 CPU, never modified."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(n_in, c_in), "w": r(KV, c_in, c_out) / (KV * c_in) ** 0.5, "b": 0.1 * r(c_out), "dy": r(n_out, c_out)}


# ------------------------------------------------------------------------------------------------------
# BasicBlock (resnet_block.py:22-57) in float64
# ------------------------------------------------------------------------------------------------------
def _conv_autograd(g, x, w):
    y = torch.zeros(g.n_out, w.shape[2], dtype=torch.float64)
    for kidx, (j, i) in enumerate(g.pairs):
        if len(j):
            y = y.index_add(0, j, x[i] @ w[kidx])
    return y


def block(g, x, p, training, eps=1e-5, momentum=0.02, masks=None):
    """conv1 - norm1 - relu - conv2 - norm2 - (+ x) - relu with autograd in float64.  ``p``: conv1.kernel, norm1.weight, norm1.bias,
    norm1.running_mean, norm1.running_var, conv2.kernel, norm2.* (float64 tensors; the running statistics are not modified).
    ``masks`` (m1, m2): the two ReLUs become multiplications by the given 0/1 masks (the GPU's own), else they are true ReLUs.
    Returns y, and the two pre-activations."""
    def bn(z, n):
        return torch.nn.functional.batch_norm(z, p[n + ".running_mean"].clone(), p[n + ".running_var"].clone(), p[n + ".weight"],
                                              p[n + ".bias"], training, momentum, eps)
    a1 = bn(_conv_autograd(g, x, p["conv1.kernel"]), "norm1")
    h = a1.clamp_min(0) if masks is None else a1 * masks[0].double()
    a2 = bn(_conv_autograd(g, h, p["conv2.kernel"]), "norm2") + x
    y = a2.clamp_min(0) if masks is None else a2 * masks[1].double()
    return y, a1, a2


@functools.lru_cache(maxsize=None)
def block_case(seed=5, n=300, c=64):
    """Point set, float32 parameters (BasicBlock names) and rows of the block tests."""
    coords = random_set(n, seed=seed)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    p = {}
    for i in (1, 2):
        p[f"conv{i}.kernel"] = r(27, c, c) / (27 * c) ** 0.5
        p[f"norm{i}.weight"] = 1 + 0.2 * r(c)
        p[f"norm{i}.bias"] = 0.3 * r(c)
        p[f"norm{i}.running_mean"] = 0.1 * r(c)
        p[f"norm{i}.running_var"] = 1 + 0.1 * r(c).abs()
    return coords, p, r(n, c), r(n, c)
