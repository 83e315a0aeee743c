"""numpy restatement of the fp16 retrieval screen (csn_amd/csrc/retrieval_screen.hip, csn_amd.minkowski_csn.topk_retrieval_ragged):
the fp32 normalisation and the 2^7 scale with the kernel's own summation order, ``numpy.float16`` rounding, float64 sums, the
bound and the selection rule.  Keep it in step with the kernel; it shares no code with it."""
import math

import numpy as np

SHIFT = 7
U, H = 2.0 ** -24, 2.0 ** -11


def padded(C):
    return (C + 31) // 32 * 32


def eps_terms(C):
    """The terms of the derived bound (DESIGN.md "fp16 screen of the shape graph"), in float64."""
    Cp = padded(C)
    d = H + (C + 8.0) * U
    return {"operands": 2.0 * d + d * d,
            "subnormal": 2.0 * 2.0 ** -21 * math.sqrt(Cp) * (1.0 + d),
            "accumulate": Cp * 2.0 * U * (1.0 + d) ** 2,
            "exact_path": (2.0 * C + 8.0) * U,
            "means": 256.0 * U}


def screen_eps(C):
    eps = sum(eps_terms(C).values()) * (1.0 + 2.0 ** -20)
    e = np.float32(eps)
    return float(e if float(e) >= eps else np.nextafter(e, np.float32(1.0)))


def accumulation_tolerance(C):
    """What the kernel may differ by from float64 sums over the SAME fp16 operands: the matrix unit's fp32 accumulation and the
    fp32 / fp64 mean of the maxima."""
    t = eps_terms(C)
    return t["accumulate"] + 16.0 * U


def image(f):
    """(N, C) fp32 rows -> (N, C) float16 image = fp16(2^7 x / max(|x|, 1e-12)), every fp32 step in the kernel's order."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    N, C = f.shape
    with np.errstate(all="ignore"):
        mx = np.zeros(N, np.float32) if C == 0 else np.fmax.reduce(np.abs(f), axis=1, initial=np.float32(0))
        e = np.clip((mx.view(np.uint32) >> 23) & 0xff, 1, 253).astype(np.uint32)
        pw = ((254 - e) << 23).astype(np.uint32).view(np.float32)
        y = f * pw[:, None]
        lanes = np.zeros((N, 64), np.float32)
        for c0 in range(0, C, 64):                      # lane l adds its channels l, l + 64, ... in turn
            w = min(64, C - c0)
            sq = (y[:, c0:c0 + w] * y[:, c0:c0 + w]).astype(np.float32)
            lanes[:, :w] = (lanes[:, :w] + sq).astype(np.float32)
        for o in (32, 16, 8, 4, 2, 1):                  # the butterfly: every lane ends with the same bits
            lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(np.float32)
        s = lanes[:, 0]
        scale = np.float32(2 ** SHIFT) / np.maximum(np.sqrt(s), np.float32(1e-12) * pw)
        return (y * scale[:, None]).astype(np.float32).astype(np.float16)


def _split(rows, off):
    return [rows[a:b] for a, b in zip(off, off[1:])]


def screen_scores(f1, off1, f2, off2):
    """(S1, S2) float64: mean_n max_m of the float64 dot of the two fp16 images, scaled back by 2^-14."""
    a = [x.astype(np.float64) for x in _split(image(f1), off1)]
    b = [x.astype(np.float64) for x in _split(image(f2), off2)]
    out = np.empty((len(a), len(b)))
    with np.errstate(all="ignore"):
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                out[i, j] = (x @ y.T).max(axis=1).mean() * 2.0 ** (-2 * SHIFT)
    return out


def exact_scores(f1, off1, f2, off2):
    """(S1, S2) float64: the measure itself in float64 on the fp32 inputs (clamp: the fp32 value of 1e-12)."""
    def unit(f):
        f = np.asarray(f, dtype=np.float64)
        return f / np.maximum(np.sqrt((f * f).sum(axis=1, keepdims=True)), float(np.float32(1e-12)))
    a, b = _split(unit(f1), off1), _split(unit(f2), off2)
    out = np.empty((len(a), len(b)))
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i, j] = (x @ y.T).max(axis=1).mean()
    return out


def shortlist(screen, k_top, eps, wild=None):
    """The selection rule: keep score >= (k_top-th largest COVERED score of the row) - 2 eps.  ``wild`` marks the candidates the
    bound does not cover: always kept, never part of the threshold.  A row with fewer than k_top covered candidates, or with a
    non-finite covered score, keeps everything."""
    s = np.asarray(screen, dtype=np.float64).copy()
    wild = np.zeros(s.shape[1], bool) if wild is None else np.asarray(wild, bool)
    bad = (~np.isfinite(s[:, ~wild])).any(axis=1, keepdims=True)
    s[:, wild] = -np.inf
    with np.errstate(invalid="ignore"):
        t = -np.sort(-s, axis=1)[:, k_top - 1:k_top]
        keep = s >= t - 2.0 * eps
    return keep | wild[None, :] | bad


def fp32_scores(f1, off1, f2, off2):
    """(S1, S2) float32: the fp32 measure as the exact kernels compute it, to rounding — fp32 sums of squares (overflowing to inf
    where the kernels' do), inverse norms with the clamp, fp32 products.  Only for inputs whose interest is that overflow."""
    def inv(f):
        with np.errstate(all="ignore"):
            s = (f.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)
            return (np.float32(1) / np.maximum(np.sqrt(s), np.float32(1e-12))).astype(np.float32)
    f1, f2 = np.asarray(f1, np.float32), np.asarray(f2, np.float32)
    i1, i2 = inv(f1), inv(f2)
    out = np.empty((len(off1) - 1, len(off2) - 1), np.float32)
    with np.errstate(all="ignore"):
        for i, (a, b) in enumerate(zip(off1, off1[1:])):
            for j, (c, d) in enumerate(zip(off2, off2[1:])):
                cos = (f1[a:b] @ f2[c:d].T) * i1[a:b, None] * i2[None, c:d]
                out[i, j] = np.fmax.reduce(cos, axis=1, initial=-np.inf).mean()
    return out


def unscreenable(rows, off, limit=2.0 ** 55):
    """(S,) bool: shapes with a non-finite element or one beyond ``limit`` (csn_amd.minkowski_csn._unscreenable)."""
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(rows).max(axis=1) <= limit)
    return np.array([bad[a:b].any() for a, b in zip(off, off[1:])])


# ---- collections the tests share (fp32 packed rows + offsets) --------------------------------------------------------------
def _pack(shapes):
    off = [0]
    for s in shapes:
        off.append(off[-1] + len(s))
    return np.concatenate(shapes).astype(np.float32), off


def clustered(rng, n_shapes, C, n_clusters=4, parts=5, lo=40, hi=120, noise=0.05):
    """Shapes of ``n_clusters`` families: a family owns ``parts`` directions, a shape's points scatter around them.  Shapes of one
    family score ~1 against each other and far lower across families."""
    dirs = rng.standard_normal((n_clusters, parts, C))
    shapes = []
    for s in range(n_shapes):
        n = int(rng.integers(lo, hi + 1))
        d = dirs[s % n_clusters][rng.integers(0, parts, n)]
        shapes.append(d * rng.uniform(0.5, 2.0, (n, 1)) + noise * rng.standard_normal((n, C)))
    return _pack(shapes)


def structureless(rng, n_shapes, C, lo=40, hi=120):
    return _pack([rng.standard_normal((int(rng.integers(lo, hi + 1)), C)) for _ in range(n_shapes)])


def near_ties(rng, n_shapes, C, n=60, rel=1e-4):
    """Perturbations, 1e-4 relative, of ONE shape: their scores differ by far less than the screen's bound."""
    base = rng.standard_normal((n, C))
    return _pack([base * (1.0 + rel * rng.standard_normal((n, C))) for _ in range(n_shapes)])


def _midpoint_element(C):
    k = math.floor(math.log2(2 ** SHIFT / math.sqrt(C)))
    if (2.0 ** k * (1 + 2.0 ** -10) / 2 ** SHIFT) ** 2 * (C - 1) >= 1.0:
        k -= 1
    return 2.0 ** k * (1.0 + 0.98 * 2.0 ** -11) / 2 ** SHIFT


def midpoint_expected_ratio(C):
    """error / eps that ``midpoint_rows`` is built to reach: the C - 1 engineered channels carry (C - 1) a^2 of a cosine of ~1 and
    lose 2 * 0.98 * 2^-11 of it (both operands rounded down)."""
    a = _midpoint_element(C)
    return (C - 1) * a * a * 2 * 0.98 * 2.0 ** -11 / screen_eps(C)


def midpoint_rows(rng, n, C):
    """Rows whose 2^7-scaled unit elements sit just UNDER an fp16 rounding midpoint at the bottom of a binade, all positive:
    C - 1 channels at T / 2^7 with T = 2^k (1 + 0.98 * 2^-11) and one channel that completes the unit norm.  Every rounded
    element is low by ~2^-11 relative, so a cosine of such rows is low by ~2 * 2^-11: the bound's leading term, nearly in full."""
    a = _midpoint_element(C)
    rest = math.sqrt(1.0 - (C - 1) * a * a)
    rows = np.full((n, C), a)
    rows[np.arange(n), rng.integers(0, C, n)] = rest
    return rows.astype(np.float32)
