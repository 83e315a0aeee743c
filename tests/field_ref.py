"""Float64 restatement of csn_amd.minkowski_field with a coordinate dictionary and no tables: quantise (both modes), interpolate,
the adjoint.  Besides the values it returns what the tests' bounds are computed from: the error scales ``sum_c w_c |z_c|`` and
``sum w |dy|`` and the number ``n_v`` of contributions per voxel.

``t = xyz - floor(xyz)`` is the FP32 difference (the module's definition: exact except for x in (-0.5, 0)); everything after it is
float64.  ``exact_t=True`` takes the float64 difference instead — what ``grid_sample`` on float64 coordinates computes."""
import numpy as np

CORNERS = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]


def _home(coords):
    c = np.asarray(coords, dtype=np.float32)
    fl = np.floor(c[:, 1:]).astype(np.int64)
    return c, np.concatenate([c[:, :1].astype(np.int64), fl], axis=1)


def quantise(coords, feats):
    """dict: voxel_coords (Nv, 4) int64 sorted by (b, x, y, z), home (Np,), vox_ptr (Nv + 1,), vox_pts (Np,), counts (Nv,),
    first (Nv, Cf) the lowest-numbered point's features, mean (Nv, Cf) float64, mean_abs (Nv, Cf) = mean |f| float64."""
    _, hv = _home(coords)
    f = np.asarray(feats, dtype=np.float64)
    cells = {}
    for p, key in enumerate(map(tuple, hv.tolist())):
        cells.setdefault(key, []).append(p)                               # ascending point numbers
    keys = sorted(cells)
    row = {k: i for i, k in enumerate(keys)}
    home = np.array([row[tuple(k)] for k in hv.tolist()], dtype=np.int64)
    counts = np.array([len(cells[k]) for k in keys], dtype=np.int64)
    return {"voxel_coords": np.array(keys, dtype=np.int64).reshape(-1, 4), "home": home,
            "vox_ptr": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            "vox_pts": np.array([p for k in keys for p in cells[k]], dtype=np.int64), "counts": counts,
            "first": np.stack([f[cells[k][0]] for k in keys]),
            "mean": np.stack([f[cells[k]].sum(0) / len(cells[k]) for k in keys]),
            "mean_abs": np.stack([np.abs(f[cells[k]]).sum(0) / len(cells[k]) for k in keys])}


def _weights(coords, exact_t=False):
    """(Np, 8) float64 corner weights in the order c = cx + 2 cy + 4 cz, and the home voxels."""
    c, hv = _home(coords)
    if exact_t:
        t = c[:, 1:].astype(np.float64) - np.floor(c[:, 1:].astype(np.float64))
    else:
        t = (c[:, 1:] - np.floor(c[:, 1:])).astype(np.float32).astype(np.float64)
    w = np.empty((c.shape[0], 8))
    for k, cr in enumerate(CORNERS):
        w[:, k] = np.prod([t[:, i] if cr[i] else 1.0 - t[:, i] for i in range(3)], axis=0)
    return w, hv


def _corner_rows(hv, voxel_coords):
    """(Np, 8) row of home + c in ``voxel_coords``, -1 where there is none (corners keep the batch index)."""
    row = {tuple(k): i for i, k in enumerate(np.asarray(voxel_coords).tolist())}
    out = np.full((hv.shape[0], 8), -1, dtype=np.int64)
    for p, (b, x, y, z) in enumerate(hv.tolist()):
        for k, (cx, cy, cz) in enumerate(CORNERS):
            out[p, k] = row.get((b, x + cx, y + cy, z + cz), -1)
    return out


def interpolate(coords, voxel_coords, z, exact_t=False):
    """(y (Np, C), scale (Np, C) = sum_c w_c |z_c|) in float64."""
    w, hv = _weights(coords, exact_t)
    rows = _corner_rows(hv, voxel_coords)
    z = np.asarray(z, dtype=np.float64)
    y = np.zeros((hv.shape[0], z.shape[1]))
    scale = np.zeros_like(y)
    for k in range(8):
        ok = rows[:, k] >= 0
        y[ok] += w[ok, k, None] * z[rows[ok, k]]
        scale[ok] += w[ok, k, None] * np.abs(z[rows[ok, k]])
    return y, scale


def adjoint(coords, voxel_coords, dy, exact_t=False):
    """(dz (Nv, C), scale (Nv, C) = sum w |dy|, n_v (Nv,) the number of (point, corner) contributions of every voxel)."""
    w, hv = _weights(coords, exact_t)
    rows = _corner_rows(hv, voxel_coords)
    dy = np.asarray(dy, dtype=np.float64)
    n_vox = np.asarray(voxel_coords).shape[0]
    dz = np.zeros((n_vox, dy.shape[1]))
    scale = np.zeros_like(dz)
    n_v = np.zeros(n_vox, dtype=np.int64)
    for k in range(8):
        ok = rows[:, k] >= 0
        np.add.at(dz, rows[ok, k], w[ok, k, None] * dy[ok])
        np.add.at(scale, rows[ok, k], w[ok, k, None] * np.abs(dy[ok]))
        np.add.at(n_v, rows[ok, k], 1)
    return dz, scale, n_v


# ------------------------------------------------------------------------------------------------------
# point sets of the tests: float32 (Np, 4) rows [b, x, y, z], sorted by shape
# ------------------------------------------------------------------------------------------------------
def random_points(n, seed=0, shapes=2, extent=6.0):
    """``n`` points in ``shapes`` shapes around the origin (negative coordinates included): clustered enough that voxels share
    points and have neighbours, sparse enough that most corners are missing somewhere."""
    rng = np.random.default_rng(seed)
    b = np.sort(rng.integers(0, shapes, size=n)) if n >= shapes else np.zeros(n, dtype=np.int64)
    b = np.unique(b, return_inverse=True)[1]                              # every shape present: 0 .. B-1 without gaps
    xyz = rng.normal(scale=extent / 3, size=(n, 3))
    return np.concatenate([b[:, None].astype(np.float64), xyz], axis=1).astype(np.float32)


def special_sets():
    """name -> (Np, 4) float32: the point sets the issue names."""
    rng = np.random.default_rng(5)
    full = np.array([[0, x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64)
    full = np.concatenate([full + [0, 0.25, 0.5, 0.75], full + [0, 0.6, 0.1, 0.9]])     # two points per voxel of a 2^3 block
    inside = np.array([[0, 0.3, 0.4, 0.7], [0, 0.9, 0.2, 0.5]])                        # home (0, 0, 0): all eight corners present
    heavy = np.concatenate([np.concatenate([np.zeros((300, 1)), rng.uniform(0, 1, size=(300, 3)) + [2, -3, 1]], axis=1),
                            np.array([[0, 1.5, -2.5, 1.5], [0, 3.5, -2.5, 1.5], [0, 2.5, -3.5, 0.5], [0, 1.25, -3.75, 0.25]])])
    edge = 32767.0
    return {
        "isolated": np.array([[0, 4.25, -7.5, 2.75]]),                                  # seven corners missing
        "full_block": np.concatenate([full, inside]),
        "shared_xyz": np.array([[0, 0.3, 1.2, -0.4], [0, 1.3, 1.2, -0.4], [1, 0.3, 1.2, -0.4], [1, 1.3, 1.2, -0.4]]),
        "lattice": np.array([[0, 2.0, -1.0, 3.0], [0, 3.0, -1.0, 3.0], [0, 2.5, -0.75, 3.5]]),     # t = 0 on every axis
        "range_edge": np.array([[0, edge + 0.5, edge + 0.25, -32768.0 + 0.5], [0, edge - 0.5, edge + 0.25, -32768.0 + 0.5],
                                [1, -32768.0, -32768.0 + 0.75, edge + 0.5]]),
        "heavy_voxel": heavy,
    }
