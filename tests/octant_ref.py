"""float64 restatement of the kernel-2 stride-2 convolution on voxel rows and its transposed form (csn_amd/minkowski_conv.py:
``build_octant_map``, ``octant_conv_down`` / ``octant_conv_up``; include/csn_hip.h section 21), written from the definitions with a
coordinate dictionary — no searchsorted, no tables:

  coarse set  sorted unique [b, floor(xyz / 2ts) 2ts] (python's // is floor), or a given list
  parent[i]   the coarse row of fine row i;  octant[i] = ox + 2 oy + 4 oz, o = (xyz - floor(xyz / 2ts) 2ts) / ts in {0, 1}^3
  down        y[j] = sum over the fine rows i with parent[i] = j of x[i] W[octant[i]]  (+ bias)
  up          y[i] = x[parent[i]] W[octant[i]]  (+ bias)

``down`` / ``up`` and their gradients walk the fine rows one by one.  The point sets are those of tests/sparse_conv_ref.py, plus one
whose y are all even (the octants with oy = 1 are empty), two dense boxes whose octant segments fill the 128-row tile exactly or miss it
by one row, and the cases that take the weight gradient past one 16-row step per wave."""
import functools

import torch

from tests import sparse_conv_ref as R


def even_y(n=200, ts=1):
    """``random_set`` with every y doubled: four empty octants."""
    return [[b, x, 2 * y, z] for b, x, y, z in R.random_set(n, ts=ts)]


def box128():
    """A dense 16 x 16 x 4 block of one shape on even corners: 1024 fine rows, 128 coarse rows, eight segments of exactly 128 rows
    (every 128-row tile exactly full, the slot behind it empty)."""
    return [[0, x, y, z] for z in range(4) for y in range(16) for x in range(16)]


def box127_129():
    """``box128`` without its last voxel (octant 7) plus one far-away voxel on an even corner (octant 0): segments
    [129, 128, 128, 128, 128, 128, 128, 127]."""
    return box128()[:-1] + [[0, 1000, 1000, 1000]]


# (point set, c_in, c_out, split-K chunk of the weight gradient by the launch rule of csn_amd/csrc/octant_conv.hip): a wave contracts
# a quarter of the chunk in 16-row steps, so chunk 128 is two steps, 192 three (a segment of rand2100 is 192 + about 70 rows: in the
# short chunk waves 0 and 1 work, wave 1 ends inside its second step, waves 2 and 3 have nothing), 256 four; 160 and 224 rows of dw
# take one row block per work-group (5 and 7 of them), 256 take four.  tests/test_cpu_ragged_head.py pins the chunks.
WGRAD_CASES = [("rand1031", 160, 256, 128), ("rand1031", 224, 256, 128), ("rand2100", 160, 256, 192), ("rand2100", 224, 256, 256),
               ("rand2100", 256, 256, 128)]
WGRAD_SETS = {"rand1031": lambda: R.random_set(1031), "rand2100": lambda: R.random_set(2100)}


def level(pts, ts, times):
    """The coordinate list ``times`` levels coarser than ``pts`` (at ts): repeated ``down_coords``."""
    pts = [tuple(int(v) for v in c) for c in pts]
    for _ in range(times):
        pts = R.down_coords(pts, ts)
        ts *= 2
    return [list(c) for c in pts], ts


class Partition:
    """parent, octant (lists over the fine rows), the coarse coordinate list and children[k][j] (-1: none) from coordinates alone."""

    def __init__(self, coords, ts=1, out_coords=None):
        fine = [tuple(int(v) for v in c) for c in coords]
        s = 2 * ts
        self.coarse = R.down_coords(fine, ts) if out_coords is None else [tuple(int(v) for v in c) for c in out_coords]
        where = {c: j for j, c in enumerate(self.coarse)}
        self.n_fine, self.n_coarse = len(fine), len(self.coarse)
        self.parent, self.octant = [], []
        self.children = [[-1] * self.n_coarse for _ in range(8)]
        for i, (b, x, y, z) in enumerate(fine):
            j = where[(b, x // s * s, y // s * s, z // s * s)]
            k = (x - x // s * s) // ts + 2 * ((y - y // s * s) // ts) + 4 * ((z - z // s * s) // ts)
            assert 0 <= k < 8 and self.children[k][j] == -1
            self.parent.append(j)
            self.octant.append(k)
            self.children[k][j] = i

    def segments(self):
        return [self.octant.count(k) for k in range(8)]


def down_fwd(p, x, w, bias=None):
    x, w = x.double(), w.double()
    y = torch.zeros(p.n_coarse, w.shape[2], dtype=torch.float64)
    for i in range(p.n_fine):
        y[p.parent[i]] += x[i] @ w[p.octant[i]]
    return y if bias is None else y + bias.double().reshape(1, -1)


def up_fwd(p, x, w, bias=None):
    x, w = x.double(), w.double()
    y = torch.zeros(p.n_fine, w.shape[2], dtype=torch.float64)
    for i in range(p.n_fine):
        y[i] = x[p.parent[i]] @ w[p.octant[i]]
    return y if bias is None else y + bias.double().reshape(1, -1)


def down_bwd(p, dy, x, w):
    dy, x, w = dy.double(), x.double(), w.double()
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for i in range(p.n_fine):
        j, k = p.parent[i], p.octant[i]
        dx[i] = dy[j] @ w[k].t()
        dw[k] += torch.outer(x[i], dy[j])
    return {"dx": dx, "dw": dw, "dbias": dy.sum(0)}


def up_bwd(p, dy, x, w):
    dy, x, w = dy.double(), x.double(), w.double()
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for i in range(p.n_fine):
        j, k = p.parent[i], p.octant[i]
        dx[j] += dy[i] @ w[k].t()
        dw[k] += torch.outer(x[j], dy[i])
    return {"dx": dx, "dw": dw, "dbias": dy.sum(0)}


@functools.lru_cache(maxsize=None)
def tensors(seed, n_in, n_out, c_in, c_out):
    """x, w (variance 1 / (8 c_in): outputs O(1)), bias, dy — float32 CPU, never modified."""
    return R.tensors(seed, n_in, n_out, 8, c_in, c_out)
