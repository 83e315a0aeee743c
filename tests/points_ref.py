"""numpy float64 restatements for csn_amd.minkowski_points (include/csn_hip.h section 18).  Two statements of one item's chain:

  (a) ``reference_item``: the order of operations of the reference's data path (MinkowskiNet/lib/dataset.py:221-252,
      lib/transforms.py:12-89, lib/voxelizer.py:34-45) — 3x3 matrix products for the rotation and the scale, the homogeneous
      product with the 4x4 voxelisation matrix (a multiplication by 1 / voxel_size), then the cast to fp32;
  (b) ``project_item``: this project's order — products and adds written out one by one, a DIVISION by the voxel size.

and two of the normalisation: ``normalize64`` (this project's, float64) and ``normalize_reference`` (the reference's, in the dtype of
its fp32 input with numpy's mean).  Written from the description of the arithmetic, not from the reference's text."""
import numpy as np

C_BITS = 16
C_BIAS = 1 << (C_BITS - 1)
EPS32 = float(np.finfo(np.float32).eps)


# ---- one item ----------------------------------------------------------------------------------------------------------------
def reference_item(xyz32, angle, shift_z, jitter, scale, sigma, clip, voxel_size, shift_on=True, jitter_on=True):
    """(a).  ``xyz32 (n, 3)`` float32.  Returns ``(q, v)`` float64: the augmented points (the features) and the voxel coordinates."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    p = np.matmul(rot, xyz32.T).T
    if shift_on:
        extent = p.max(axis=0) - p.min(axis=0)
        length = np.sqrt(np.sum(extent ** 2))
        p = p + np.clip((sigma * length) * np.asarray(shift_z, dtype=np.float64).reshape(1, 3), -clip, clip)
    if jitter_on:
        p = np.asarray(jitter, dtype=np.float64).reshape(1, 3) + p
    p = np.matmul(np.diag([scale, scale, scale]), p.T).T
    m = np.eye(4)
    m[0, 0] = m[1, 1] = m[2, 2] = 1 / voxel_size
    homo = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1)
    return p, homo @ m.T[:, :3]


def bounds_item(xyz32, angle):
    """(18b): the rotated points (float64) and their extent per axis."""
    c, s = np.cos(angle), np.sin(angle)
    x, y, z = (xyz32[:, k].astype(np.float64) for k in range(3))
    r = np.stack([c * x + s * z, y, (-s) * x + c * z], axis=1)
    return r, r.max(axis=0) - r.min(axis=0)


def project_item(xyz32, angle, shift_z, jitter, scale, sigma, clip, voxel_size):
    """(b).  Returns ``(q, v)`` float64 as ``reference_item`` does.  Every numpy operation below rounds once; none is fused."""
    r, e = bounds_item(xyz32, angle)
    diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    t = np.clip((sigma * diag) * np.asarray(shift_z, dtype=np.float64), -clip, clip)
    q = ((r + t[None, :]) + np.asarray(jitter, dtype=np.float64)[None, :]) * scale
    return q, q / voxel_size


def pack(b, fl):
    fl = fl.astype(np.int64)
    return (np.int64(b) << (3 * C_BITS)) | ((fl[:, 0] + C_BIAS) << (2 * C_BITS)) | ((fl[:, 1] + C_BIAS) << C_BITS) | (fl[:, 2] + C_BIAS)


def project_batch(shapes, labels, indices, params, sigma, clip, voxel_size):
    """(b) for a whole batch: what ``PointCollection.batch`` returns, as numpy arrays.  ``params``: an ``AugmentParams`` or anything
    with ``angle``, ``shift_z``, ``jitter``, ``scale``."""
    coords, feats, keys, labs, off = [], [], [], [], [0]
    for i, s in enumerate(indices):
        q, v = project_item(shapes[s], params.angle[i], params.shift_z[i], params.jitter[i], params.scale[i], sigma, clip, voxel_size)
        v32 = v.astype(np.float32)
        coords.append(np.concatenate([np.full((v32.shape[0], 1), i, dtype=np.float32), v32], axis=1))
        feats.append(q.astype(np.float32))
        keys.append(pack(i, np.floor(v32)))
        if labels is not None:
            labs.append(np.asarray(labels[s]).reshape(-1).astype(np.int64))
        off.append(off[-1] + v32.shape[0])
    return {"coords": np.concatenate(coords), "feats": np.concatenate(feats), "keys": np.concatenate(keys),
            "labels": np.concatenate(labs) if labs else None, "offsets": np.asarray(off, dtype=np.int64)}


# ---- normalisation -----------------------------------------------------------------------------------------------------------
def normalize64(xyz32, method="sphere"):
    """This project's statement, float64 on the fp32 input: ``(p - c) / r`` (float64; the kernel stores its fp32 rounding)."""
    p = xyz32.astype(np.float64)
    d = p - p.sum(axis=0) / p.shape[0]
    if method == "sphere":
        r = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    else:
        e = d.max(axis=0) - d.min(axis=0)
        r = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return d / max(r, 2.0 * EPS32)


def normalize_reference(xyz32, method="sphere"):
    """The reference's order in the input's own dtype (fp32 for a prefetched category): numpy's mean, the norm by sum of squares."""
    d = xyz32 - np.mean(xyz32, axis=0)
    if method == "sphere":
        r = np.max(np.sqrt(np.sum(d ** 2, axis=1)))
    else:
        r = np.sqrt(np.sum((d.max(axis=0) - d.min(axis=0)) ** 2))
    return d / np.maximum(r, 2.0 * np.finfo(d.dtype).eps)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def ulp32_distance(a, b):
    """Per element, how many fp32 values lie between the fp32 arrays a and b (0: the same bits or +0 / -0)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def random_shapes(n_shapes, n_points, seed=0):
    """Normalised-looking shapes: points in the unit ball, anisotropic, as fp32."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_shapes):
        n = n_points[s] if not np.isscalar(n_points) else n_points
        p = rng.standard_normal((n, 3)) * np.array([0.5, 0.3, 0.4])
        p = p / max(1.0, np.abs(p).max() / 0.9)
        out.append(np.ascontiguousarray(p, dtype=np.float32))
    return out


# ---- the raw entry points' host-side rejections.  The non-NULL pointers are host buffers that are never dereferenced: EVERY call below
# must be refused before any launch (a call that is meant to pass one check carries a misaligned pointer for the next) ----
def abi_rejections(L):
    import ctypes
    ARG, PTR, DIM = -1, -3, -5
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    norm = lambda pts=p, off=p, ns=2, nt=5, m=0, out=p, st=p: L.csn_points_normalize_f32(pts, off, ns, nt, m, out, st, None)
    bnd = lambda pts=p, off=p, ns=2, nt=5, idx=p, par=p, ni=2, b=p, st=p: L.csn_points_bounds_f64(pts, off, ns, nt, idx, par, ni, b, st, None)
    bat = lambda pts=p, lab=p, off=p, ns=2, nt=5, idx=p, oo=p, par=p, b=p, ni=2, mp=3, sg=0.01, cl=0.05, vs=0.05, co=p, fe=p, lo=p, k=p, no=5, st=p: \
        L.csn_points_batch_f32(pts, lab, off, ns, nt, idx, oo, par, b, ni, mp, sg, cl, vs, co, fe, lo, k, no, st, None)
    fidx = lambda sk=p, od=p, vid=p, n=4, nv=2, h=p, vp=p, vq=p, u=p, st=p: L.csn_field_index_i32(sk, od, vid, n, nv, h, vp, vq, u, st, None)
    for fn, names in ((norm, ("pts", "off", "out", "st")), (bnd, ("pts", "off", "idx", "par", "b", "st")),
                      (bat, ("pts", "off", "idx", "oo", "par", "b", "co", "fe", "k", "st", "lo")),
                      (fidx, ("sk", "od", "vid", "h", "vp", "vq", "u", "st"))):
        for name in names:
            assert fn(**{name: None}) == ARG, name
    assert bat(lab=None, co=p + 8) == PTR and bat(lab=None, lo=None, co=p + 8) == PTR    # labels are optional, labels_out with them
    for fn in (norm, bnd, bat):
        assert fn(ns=0) == ARG and fn(nt=0) == ARG and fn(ns=-1) == ARG
    assert norm(m=2) == ARG and norm(m=-1) == ARG
    assert bnd(ni=0) == ARG and bat(ni=0) == ARG and bat(mp=0) == ARG and bat(no=0) == ARG
    for bad in (0.0, -0.05, float("nan")):
        assert bat(vs=bad) == ARG and bat(cl=bad) == ARG
    assert bat(sg=-1.0) == ARG and bat(sg=float("nan")) == ARG and bat(sg=0.0, co=p + 8) == PTR
    assert fidx(n=0) == ARG and fidx(nv=0) == ARG
    assert bat(ni=65536) == DIM and bat(ni=65535, co=p + 8) == PTR and fidx(n=4, nv=5) == DIM
    assert bat(ni=65536, vs=0.0) == ARG                                        # a bad argument is named before a bad size
    assert norm(pts=p + 2) == PTR and norm(off=p + 4) == PTR and norm(out=p + 1) == PTR and norm(st=p + 2) == PTR
    assert bnd(idx=p + 4) == PTR and bnd(par=p + 4) == PTR and bnd(b=p + 4) == PTR
    assert bat(co=p + 8) == PTR and bat(fe=p + 2) == PTR and bat(k=p + 4) == PTR and bat(lab=p + 2) == PTR and bat(lo=p + 4) == PTR
    assert bat(oo=p + 4) == PTR and bat(co=p + 8, ni=65536) == DIM              # ... and a bad size before a bad pointer
    assert fidx(sk=p + 4) == PTR and fidx(od=p + 4) == PTR and fidx(vid=p + 4) == PTR and fidx(u=p + 4) == PTR
    assert fidx(h=p + 2) == PTR and fidx(vp=p + 2) == PTR and fidx(vq=p + 2) == PTR and fidx(st=p + 2) == PTR
