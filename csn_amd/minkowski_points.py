"""Resident point collections: a category's points on the device; normalised once, then augmented, voxel-scaled, keyed and collated
per batch by the kernels of include/csn_hip.h section 18.

Reference (marios2019/CSN), the stage in front of ``batch_points``:
  * the prefetched category and its per-shape normalisation            MinkowskiNet/lib/dataset.py:104-126, lib/transforms.py:195-225
  * ``__getitem__``: angle, prevoxel transforms, coordinates as features, ``Voxelizer.voxelize``     lib/dataset.py:221-252
  * rotation about y, shift, jitter, scale                            lib/transforms.py:12-89
  * the voxel scaling                                                 lib/voxelizer.py:34-45
  * PartNet's bounds, ``--distort_partnet``                            lib/datasets/partnet.py:33-42, lib/config.py:147-152
  * ``get_neighbors``                                                  lib/csn_utils.py:114-130

The reference keeps the category in host memory and runs that chain in numpy per item and step, for (K + 1) B shapes; here the category
is ONE flat ``(N, 3)`` fp32 tensor plus offsets on the device, and a batch is two uploads (the items, their drawn numbers), two launches
(the bounding boxes of the rotated items; everything else per point) and no host read.  ``PointBatch.field()`` then builds the
``PointField`` through ``PointField.from_keys``: one sort, one scan, ONE host read, one launch.

THE ARITHMETIC (this project's statement; tests/points_ref.py restates it and the reference's order in numpy): float64 on the fp32
points, every operation rounded on its own, for item i with the drawn numbers (angle, shift_z, jitter, scale)
    c, s  = cos(angle), sin(angle)                                  on the host (numpy)
    r     = (c x + s z,  y,  (-s) x + c z)                           each product rounded, then one add
    e     = max r - min r per axis;   diag = sqrt((ex ex + ey ey) + ez ez)
    t     = clip((sigma diag) shift_z, -clip, +clip)
    q     = ((r + t) + jitter) scale
    feats = fp32(q);   coords = [fp32(i), fp32(q / voxel_size)];   keys = packed [i, floor(coords xyz)]
Disabled transforms enter with their neutral numbers (angle 0, shift_z 0, jitter 0, scale 1) and change no bit: identity parameters
give ``batch_points``'s tensors.  Normalisation: ``c = (sum p) / n``, ``r`` the bounding-sphere radius or bounding-box diagonal of
``p - c``, at least 2 eps_fp32, ``fp32((p - c) / r)`` — float64 throughout (the reference: fp32 with numpy's mean).

The drawn numbers are CPU float64 arrays from a ``numpy.random.Generator`` in the reference's per-item order.  The reference draws
from numpy's global state inside data-loader workers: no parity with its stream exists or is claimed — same numbers in, same points
out.  Out of scope: sampling and shuffling policy, rotation of normals (PartNet runs on xyz features alone).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import functional as CF
from .minkowski_conv import _B_BITS
from .minkowski_field import PointField

_NO_CPU = "csn_amd ops need tensors on the MI355X (cuda) device; there is no CPU path"
N_PARAM = 9                                  # per item: cos, sin, shift_z[3], jitter[3], scale (include/csn_hip.h section 18)
MAX_ITEMS = 65535                            # csn_points_batch_f32: one grid row per item
NORMALIZE_METHODS = ("sphere", "box")


@dataclass
class AugmentParams:
    """The drawn numbers of n items, CPU float64: ``angle (n,)``, ``shift_z (n, 3)`` standard normals, ``jitter (n, 3)``,
    ``scale (n,)``."""
    angle: np.ndarray
    shift_z: np.ndarray
    jitter: np.ndarray
    scale: np.ndarray

    def __post_init__(self):
        self.angle = np.ascontiguousarray(self.angle, dtype=np.float64).reshape(-1)
        n = self.angle.shape[0]
        self.shift_z = np.ascontiguousarray(self.shift_z, dtype=np.float64)
        self.jitter = np.ascontiguousarray(self.jitter, dtype=np.float64)
        self.scale = np.ascontiguousarray(self.scale, dtype=np.float64).reshape(-1)
        if self.shift_z.shape != (n, 3) or self.jitter.shape != (n, 3) or self.scale.shape != (n,):
            raise ValueError("AugmentParams: angle (n,), shift_z (n, 3), jitter (n, 3), scale (n,) for one n")

    def __len__(self) -> int:
        return self.angle.shape[0]

    @staticmethod
    def identity(n: int) -> "AugmentParams":
        """The neutral numbers for n items: nothing moves, no bit changes."""
        return AugmentParams(np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.ones(n))

    def slice(self, lo: int, hi: int) -> "AugmentParams":
        return AugmentParams(self.angle[lo:hi], self.shift_z[lo:hi], self.jitter[lo:hi], self.scale[lo:hi])

    def packed(self) -> np.ndarray:
        """``(n, 9)`` float64: cos, sin, shift_z, jitter, scale — the ``params`` rows of section 18."""
        out = np.empty((len(self), N_PARAM), dtype=np.float64)
        out[:, 0], out[:, 1] = np.cos(self.angle), np.sin(self.angle)
        out[:, 2:5], out[:, 5:8], out[:, 8] = self.shift_z, self.jitter, self.scale
        return out


@dataclass
class AugmentSpec:
    """Which transforms run and their bounds; the defaults are PartNet's (partnet.py:36-42).  The reference applies shift XOR jitter
    (dataset.py:278-281); a spec may switch both on, the order of the module docstring covers it."""
    rotation_bound: Tuple[float, float] = (-5 * math.pi / 180.0, 5 * math.pi / 180)
    jitter_bound: Tuple[float, float, float] = (0.25, 0.25, 0.25)
    scale_bound: Tuple[float, float] = (0.75, 1.25)
    shift: Tuple[float, float] = (0.01, 0.05)                          # (sigma, clip)
    rotate: bool = False
    shift_on: bool = False
    jitter_on: bool = False
    scale_on: bool = False

    def __post_init__(self):
        if len(self.rotation_bound) != 2 or len(self.jitter_bound) != 3 or len(self.scale_bound) != 2 or len(self.shift) != 2:
            raise ValueError("AugmentSpec: rotation_bound (lo, hi), jitter_bound (x, y, z), scale_bound (lo, hi), shift (sigma, clip)")
        if not self.shift[0] >= 0 or not self.shift[1] > 0:
            raise ValueError("AugmentSpec: shift needs sigma >= 0 and clip > 0")

    @staticmethod
    def distort_partnet() -> "AugmentSpec":
        """``--distort_partnet`` (config.py:147-152): random rotation, jitter and scale; no shift."""
        return AugmentSpec(rotate=True, jitter_on=True, scale_on=True, shift_on=False)

    def draw(self, n: int, rng: np.random.Generator) -> AugmentParams:
        """The numbers of n items, drawn item by item in the reference's order: the angle (dataset.py:224), the three shift normals,
        jitter x, y, z, the scale (transforms.py:26, 42, 57).  A disabled transform draws nothing and gives its neutral number."""
        p = AugmentParams.identity(n)
        for i in range(n):
            if self.rotate:
                p.angle[i] = rng.uniform(self.rotation_bound[0], self.rotation_bound[1])
            if self.shift_on:
                p.shift_z[i] = rng.standard_normal(3)
            if self.jitter_on:
                for k in range(3):
                    p.jitter[i, k] = rng.uniform(-self.jitter_bound[k], self.jitter_bound[k])
            if self.scale_on:
                p.scale[i] = rng.uniform(self.scale_bound[0], self.scale_bound[1])
        return p


class PointBatch:
    """A collated batch on the device: ``coords (Np, 4)`` float32 ``[b, x, y, z]`` in voxel units, ``feats (Np, 3)`` float32 (the
    augmented coordinates before the voxel scaling), ``labels (Np,)`` int64 or None, ``keys (Np,)`` int64 (the packed key of
    ``[b, floor(x), floor(y), floor(z)]``, include/csn_hip.h section 17), ``status (1,)`` int32 (section 18's word, still on the
    device: ``field()`` reads it), ``offsets (B + 1,)`` int64 on the host — known from the collection without a device read."""

    def __init__(self, coords, feats, labels, keys, status, offsets):
        self.coords, self.feats, self.labels, self.keys, self.status, self.offsets = coords, feats, labels, keys, status, offsets
        self.group_shapes = None           # PointCollection.merged_batch: the shapes of every group of a merged batch

    @property
    def n_points(self) -> int:
        return self.coords.shape[0]

    @property
    def n_shapes(self) -> int:
        return self.offsets.numel() - 1

    def field(self, quantization_mode: str = "random_subsample") -> PointField:
        """The ``PointField`` of the batch (``PointField.from_keys``); a flagged batch raises ``ValueError`` here."""
        return PointField.from_keys(self.coords, self.feats, self.keys, self.status, self.offsets, quantization_mode)


class PointCollection:
    """A category on the device: ``points`` as an ``(S, P, 3)`` float32 array or a list of ``(n_i, 3)`` float32 arrays (numpy or
    torch), ``labels`` alike as ``(S, P)`` / a list of ``(n_i,)`` integers.  Kept flat: ``points (N, 3)`` float32 and ``labels (N,)``
    int32 on the device, ``offsets (S + 1,)`` int64 on both sides (``offsets`` host, ``offsets_dev``).  ``device="cpu"`` holds the
    data and checks arguments; ``normalize`` and ``batch`` then raise ``CsnError``: there is no CPU path."""

    def __init__(self, points, labels=None, device="cuda"):
        device = torch.device(device)                  # "cpu" holds the data for host-side preparation; every op needs the device
        shapes = self._as_list(points, "points", np.float32, 3)
        counts = [s.shape[0] for s in shapes]
        self.offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
        if labels is not None:
            labs = self._as_list(labels, "labels", None, None)
            if [l.shape[0] for l in labs] != counts:
                raise ValueError("labels must bring one integer per point of every shape")
            flat = np.concatenate(labs)
            if flat.size and (flat.min() < -2 ** 31 or flat.max() >= 2 ** 31):
                raise ValueError("labels must fit int32")
            self.labels = torch.from_numpy(flat.astype(np.int32)).to(device)
        else:
            self.labels = None
        self.points = torch.from_numpy(np.ascontiguousarray(np.concatenate(shapes))).to(device)
        self.offsets_dev = self.offsets.to(device)
        self.normalized: Optional[str] = None

    @staticmethod
    def _as_list(data, what, dtype, width):
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        items = list(data) if not isinstance(data, np.ndarray) else ([data[i] for i in range(data.shape[0])] if data.ndim == (3 if width else 2) else None)
        if not items:
            raise ValueError(f"{what} must be an (S, P{', 3' if width else ''}) array or a non-empty list of per-shape arrays")
        out = []
        for a in items:
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            if width:
                if a.ndim != 2 or a.shape[1] != width or a.shape[0] < 1 or a.dtype != dtype:
                    raise ValueError(f"{what}: every shape is a non-empty (n, {width}) {np.dtype(dtype).name} array")
            else:
                a = a.reshape(-1) if a.ndim == 2 and a.shape[1] == 1 else a
                if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"{what}: every shape is an (n,) integer array")
            out.append(a)
        return out

    @classmethod
    def from_h5_files(cls, paths: Sequence[str], root: str = "", device="cuda") -> "PointCollection":
        """The PartNet layout of dataset.py:132-146: every file holds ``data (S, P, 3)`` and ``label_seg (S, P)``; the files are
        stacked in the order given.  Needs ``h5py``."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError("PointCollection.from_h5_files needs the h5py package, which is not installed") from e
        import os
        pts, labs = [], []
        for p in paths:
            with h5py.File(os.path.join(root, p), "r") as f:
                pts.append(f["data"][:].astype(np.float32))
                lab = f["label_seg"][:].astype(np.int32)
                labs.append(lab.reshape(pts[-1].shape[0], -1))
        return cls(np.concatenate(pts), np.concatenate(labs), device=device)

    # ---- sizes ----
    @property
    def n_shapes(self) -> int:
        return self.offsets.numel() - 1

    @property
    def n_points(self) -> int:
        return self.points.shape[0]

    @property
    def device(self) -> torch.device:
        return self.points.device

    def to(self, device) -> "PointCollection":
        """The collection on ``device``: the arrays move, nothing is recomputed."""
        c = object.__new__(PointCollection)
        c.offsets, c.normalized = self.offsets, self.normalized
        c.points, c.offsets_dev = self.points.to(device), self.offsets.to(device)
        c.labels = None if self.labels is None else self.labels.to(device)
        return c

    def _need_device(self) -> None:
        if not self.points.is_cuda:
            raise _lib.CsnError(_NO_CPU)

    def _new_status(self) -> torch.Tensor:
        return torch.zeros(1, dtype=torch.int32, device=self.device)

    # ---- once: normalisation ----
    def normalize(self, method: str = "sphere") -> "PointCollection":
        """``normalize_coords`` (transforms.py:195-225) on every shape, in place, once (``csn_points_normalize_f32``)."""
        if method not in NORMALIZE_METHODS:
            raise ValueError(f"method must be one of {NORMALIZE_METHODS}")
        self._need_device()
        status = self._new_status()
        _lib.check(_lib.lib().csn_points_normalize_f32(CF._ptr(self.points), CF._ptr(self.offsets_dev), self.n_shapes, self.n_points,
                                                       NORMALIZE_METHODS.index(method), CF._ptr(self.points), CF._ptr(status),
                                                       CF._stream()), "csn_points_normalize_f32")
        self.normalized = method
        return self

    # ---- per step: a batch ----
    def _indices(self, indices) -> np.ndarray:
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("indices must be a non-empty sequence of shape numbers")
        if idx.min() < 0 or idx.max() >= self.n_shapes:
            raise ValueError(f"a shape number lies outside the collection's [0, {self.n_shapes})")
        if idx.size > min(MAX_ITEMS, 1 << _B_BITS):
            raise ValueError(f"a batch holds at most {min(MAX_ITEMS, 1 << _B_BITS)} items")
        return idx.astype(np.int64)

    def batch(self, indices, params: Optional[AugmentParams] = None, voxel_size: float = 0.05,
              shift: Tuple[float, float] = (0.01, 0.05)) -> PointBatch:
        """The collated batch of the shapes ``indices`` (repeats and any order are fine), item i augmented with row i of ``params``
        (None: identity, which reproduces ``batch_points`` bit for bit).  ``shift`` = (sigma, clip) of the spec that drew
        ``params``.  Two launches: ``csn_points_bounds_f64``, ``csn_points_batch_f32``; no host read — the status word travels with
        the batch."""
        idx = self._indices(indices)
        n = idx.size
        if not (isinstance(voxel_size, (int, float)) and voxel_size > 0 and math.isfinite(voxel_size)):
            raise ValueError("voxel_size must be a positive number")
        if params is None:
            params = AugmentParams.identity(n)
        if len(params) != n:
            raise ValueError(f"params hold {len(params)} items, the batch {n}")
        sigma, clip = float(shift[0]), float(shift[1])
        if not sigma >= 0 or not clip > 0:
            raise ValueError("shift needs sigma >= 0 and clip > 0")
        self._need_device()
        host_off = self.offsets.numpy()
        counts = host_off[idx + 1] - host_off[idx]
        out_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n_out = int(out_off[-1])
        dev = self.device
        items = torch.from_numpy(np.stack([idx, out_off[:-1]])).to(dev)             # (2, n) int64: one upload
        par = torch.from_numpy(params.packed()).to(dev)
        bounds = torch.empty((n, 6), dtype=torch.float64, device=dev)
        coords = torch.empty((n_out, 4), dtype=torch.float32, device=dev)
        feats = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
        keys = torch.empty(n_out, dtype=torch.int64, device=dev)
        labels = None if self.labels is None else torch.empty(n_out, dtype=torch.int64, device=dev)
        status = self._new_status()
        L = _lib.lib()
        _lib.check(L.csn_points_bounds_f64(CF._ptr(self.points), CF._ptr(self.offsets_dev), self.n_shapes, self.n_points, CF._ptr(items[0]),
                                           CF._ptr(par), n, CF._ptr(bounds), CF._ptr(status), CF._stream()), "csn_points_bounds_f64")
        _lib.check(L.csn_points_batch_f32(CF._ptr(self.points), CF._ptr(self.labels), CF._ptr(self.offsets_dev), self.n_shapes,
                                          self.n_points, CF._ptr(items[0]), CF._ptr(items[1]), CF._ptr(par), CF._ptr(bounds), n,
                                          int(counts.max()), sigma, clip, float(voxel_size), CF._ptr(coords), CF._ptr(feats),
                                          CF._ptr(labels), CF._ptr(keys), n_out, CF._ptr(status), CF._stream()), "csn_points_batch_f32")
        return PointBatch(coords, feats, labels, keys, status, torch.from_numpy(out_off))

    def neighbor_batches(self, neighbors: Sequence[Tuple[int, Sequence[int]]], K: int, params: Optional[AugmentParams] = None,
                         voxel_size: float = 0.05, shift: Tuple[float, float] = (0.01, 0.05)) -> List[PointBatch]:
        """``get_neighbors`` (csn_utils.py:114-130) on ``construct_shape_graph``'s ``[(q_idx, [neighbours])]``: K batches, batch i
        holding the i-th neighbour of every query in query order.  ``params`` covers all K B items — rows ``[i B, (i + 1) B)`` go to
        batch i — since the reference augments every neighbour on its own."""
        if K < 1:
            raise ValueError("K must be >= 1")
        B = len(neighbors)
        if B < 1:
            raise ValueError("neighbors must hold at least one query")
        for _, nbrs in neighbors:
            if len(nbrs) < K:
                raise ValueError(f"every query needs at least K = {K} neighbours")
        if params is not None and len(params) != K * B:
            raise ValueError(f"params hold {len(params)} items, the K batches {K * B}")
        for i in range(K):
            self._indices([int(nbrs[i]) for _, nbrs in neighbors])
        return [self.batch([int(nbrs[i]) for _, nbrs in neighbors], None if params is None else params.slice(i * B, (i + 1) * B),
                           voxel_size, shift) for i in range(K)]

    def merged_batch(self, indices, neighbors: Sequence[Tuple[int, Sequence[int]]], K: int, params: Optional[AugmentParams] = None,
                     voxel_size: float = 0.05, shift: Tuple[float, float] = (0.01, 0.05)) -> PointBatch:
        """The queries ``indices`` and their K neighbour batches as ONE batch of (K + 1) B items, in the per-item order of ``batch``
        followed by ``neighbor_batches``: the B queries, then the rank-0 neighbour of every query in query order, then rank 1, ...
        — item numbers (the batch column) run on, so its voxel coordinates are already the merged coordinate set of
        ``csn_amd.minkowski_hrnet.group_pyramid`` with ``n_shapes = batch.group_shapes`` ( = [B] * (K + 1)): a grouped pass
        (``HRNetSimCSN.forward((GroupedPyramid, feats))``) without K + 1 collations.  ``params`` covers all (K + 1) B items, the
        queries' first.  Still two launches and no host read."""
        if K < 1:
            raise ValueError("K must be >= 1")
        idx = [int(i) for i in self._indices(indices)]
        B = len(idx)
        if len(neighbors) != B:
            raise ValueError("neighbors must hold one entry per query")
        for _, nbrs in neighbors:
            if len(nbrs) < K:
                raise ValueError(f"every query needs at least K = {K} neighbours")
        if params is not None and len(params) != (K + 1) * B:
            raise ValueError(f"params hold {len(params)} items, the K + 1 batches {(K + 1) * B}")
        out = self.batch(idx + [int(nbrs[i]) for i in range(K) for _, nbrs in neighbors], params, voxel_size, shift)
        out.group_shapes = [B] * (K + 1)
        return out
