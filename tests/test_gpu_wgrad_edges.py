"""Weight gradients through the C ABI at every tile, chunk and accumulate edge: csn_project_wgrad_f32 and the dW of
csn_outproj_ln_bwd_f32 are one host routine (wgrad() in csn_amd/csrc/csn_capi.hip) — equal chunks of points, a split-K product
with a k-contiguous B operand into one slab per (map, chunk), then csn_slab_reduce_kernel: dw = scale * sum(slabs) (+ dw).

Every case is compared with float64 on the host.  Every buffer the call may touch is carved out of ONE allocation that is NaN
everywhere else: the pad columns n_points .. ld and the skipped slots of both input maps, a guard band behind every buffer (and in
front of it where the call is handed a pointer offset), the whole workspace, and dw itself unless the call accumulates.  A read
outside the valid points is so a NaN in dw, not a small error; a slab element that was never written is a NaN in dw; a write
outside dw or outside the csn_wgrad_workspace_floats floats of the workspace is a number in a guard.

Kernel instance per (rows, channels), k-contiguous B:
  math mode 0        rows <= 64: fp32 64 x 128            else: fp32 128 x 128
  math mode 1        rows >= 192 and channels >= 224: bf16x3 256 x 256 on 16 waves (on 8 waves with CSN_DEV_WIDE_FORMS bit 4
                     cleared, 128 x 128 with CSN_DEV_BIG_TILES = 0); else rows <= 64: bf16x3 64 x 128; else: bf16x3 128 x 128
  math modes 2, 3    the mode-1 choice with one product per pair; 256 x 256 always on 8 waves
Tolerances are the ones the suite asserts for this product (test_gpu_kernels.test_project_wgrad): 5e-6 of max |ref| in mode 0,
eight times that in mode 1; the multi-chunk cases also hold every element to tol * sum_n |a| |b|, where one wrong row cannot hide
behind the largest element."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALIGN = -2
TOL = {0: 5e-6, 1: 8 * 5e-6, 2: 5e-6, 3: 5e-6}         # modes 2 / 3: against the product of the ROUNDED operands (see _operands)
GUARD = 4096                                           # floats of NaN behind (and in front of) every buffer
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from csn_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(autouse=True)
def _switches_restored(L):
    """Math mode and every development switch a case may touch are what they were when the case ends, pass or fail."""
    lib = L.lib()
    keys = (L.DEV_BIG_TILES, L.DEV_WIDE_GEMM, L.DEV_WIDE_FORMS, L.DEV_WX)
    saved = [lib.csn_dev_get(k) for k in keys]
    try:
        yield
    finally:
        for k, v in zip(keys, saved):
            lib.csn_dev_set(k, v)
        lib.csn_set_math_mode(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _carve(n, front=0):
    """n floats inside one NaN-filled allocation: (pool, view of the n floats, guard in front, guard behind)."""
    pool = torch.full((front + n + GUARD,), NAN, device="cuda")
    return pool, pool[front:front + n], pool[:front], pool[front + n:]


def _padded(valid, ld, step=1):
    """valid: (S, rows, n) on the host -> device maps [S * step][rows][ld] whose slots 0, step, 2 step .. hold `valid` in their
    first n columns; pad columns, skipped slots and a guard band behind are NaN."""
    S, rows, n = valid.shape
    host = torch.full((S * step, rows, ld), NAN)
    host[::step, :, :n] = valid
    pool, buf, _, guard = _carve(host.numel())
    buf.copy_(host.reshape(-1))
    return pool, buf, guard


@functools.lru_cache(maxsize=None)
def _operands(S, R, C, NP, rounded=0):
    """Host operands dout (S, R, NP), x (S, C, NP) and, in float64, G = sum_{s,n} dout x and T = sum_{s,n} |dout| |x|.
    rounded = 2 / 3: G and T of the operands rounded to bf16 / fp16, which is what the single-product modes multiply (fp32 ->
    16 bits is a round to nearest even in csn_mode::to16x4, as in torch); what remains against them is fp32 accumulation."""
    rng = np.random.default_rng(1000 * R + 10 * C + NP + S)
    a = torch.from_numpy(rng.standard_normal(size=(S, R, NP)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(size=(S, C, NP)).astype(np.float32))
    ar, br = a, b
    if rounded == 2:
        ar, br = a.bfloat16(), b.bfloat16()
    elif rounded == 3:
        ar, br = a.half(), b.half()
    G = torch.einsum("srn,scn->rc", ar.double(), br.double())
    T = torch.einsum("srn,scn->rc", ar.double().abs(), br.double().abs())
    return a, b, G, T


def _slabs(L, R, C, S, NP):
    n = L.lib().csn_wgrad_workspace_floats(R, C, S, NP)
    assert n > 0 and n % (S * R * C) == 0
    return n, n // (S * R * C)


def _wgrad(L, a, b, R, C, NP, *, pad_a=4, pad_x=12, step=1, scale=1.0, accumulate=0, prefill=None, calls=1, keep_ws=False):
    """csn_project_wgrad_f32 on guarded buffers.  Returns dw on the host (and the workspace slabs with keep_ws)."""
    lib = L.lib()
    S = a.shape[0]
    lda, ldx = NP + pad_a, NP + pad_x
    _, ad, a_guard = _padded(a, lda, step)
    _, xd, x_guard = _padded(b, ldx, step)
    ws_n, _ = _slabs(L, R, C, S, NP)
    _, ws, _, ws_guard = _carve(ws_n)                             # exactly the floats the library asks for
    _, dw, _, dw_guard = _carve(R * C)                            # dw ends its allocation's payload: the guard follows at once
    if prefill is not None:
        dw.copy_(prefill.reshape(-1))
    else:
        assert accumulate == 0
    for _ in range(calls):
        L.check(lib.csn_project_wgrad_f32(ad.data_ptr(), step * R * lda, lda, xd.data_ptr(), step * C * ldx, ldx, dw.data_ptr(), R, C, S,
                                          NP, scale, accumulate, ws.data_ptr(), ws_n, _stream()), "csn_project_wgrad_f32")
    torch.cuda.synchronize()
    for g in (a_guard, x_guard, ws_guard, dw_guard):
        assert torch.isnan(g).all()                               # not one float of a guard changed
    got = dw.view(R, C).cpu()
    return (got, ws.cpu()) if keep_ws else got


def _check(got, ref, T, mode, elementwise=False, what=""):
    assert not torch.isnan(got).any(), f"{what}: NaN in dw (a read outside the valid points, or a slab element never written)"
    err = (got.double() - ref).abs()
    rel = (err.max() / ref.abs().max()).item()
    print(f"{what} mode {mode}: max-norm error {rel:.3e} (bound {TOL[mode]:.1e})", end="")
    if elementwise:
        worst = (err / T).max().item()
        print(f", elementwise error / sum |a||b| {worst:.3e}", end="")
    print()
    assert rel < TOL[mode], what
    if elementwise:
        assert bool((err <= TOL[mode] * T).all()), what


# ---- 1. tile edges, one chunk (n_points <= 256: K = n_points) ------------------------------------------------------------------
ONE_CHUNK = [
    # rows, channels, n_points, n_maps      instance in mode 0 / mode 1                       edges
    (32, 32, 4, 1),        # 64x128 / 64x128                    one chunk of 4 points, the smallest call there is
    (36, 100, 12, 3),      # 64x128 / 64x128                    M tail 4 rows into the second 32, N tail, K inside a slab
    (64, 132, 36, 9),      # 64x128 / 64x128                    full row tile, last column tile 4 wide, K = 32 + 4, 9 maps
    (32, 260, 252, 1),     # 64x128 / 64x128                    three column tiles (last 4 wide), K ends 4 short of a slab
    (36, 224, 132, 3),     # 64x128 / 64x128                    M tail, N tail of 96, K = 4 slabs + 4
    (72, 32, 256, 1),      # 128x128 / 128x128                  one row tile of 72, whole slabs
    (96, 132, 4, 9),       # 128x128 / 128x128                  K = 4, last column tile 4 wide, 9 maps
    (96, 100, 36, 1),      # 128x128 / 128x128                  M, N and K tails together
    (200, 100, 132, 3),    # 128x128 / 128x128                  two row tiles, the last of 72
    (200, 132, 252, 1),    # 128x128 / 128x128                  two row tiles x two column tiles (72 x 4 corner)
    (72, 260, 36, 3),      # 128x128 / 128x128                  three column tiles, last 4 wide (rows < 192: not the big tile)
    (200, 224, 12, 9),     # 128x128 / 256x256 (16 waves)       one short tile: 200 rows, 224 columns, K = 12, 9 maps
    (200, 260, 4, 3),      # 128x128 / 256x256                  K = 4, last column tile 4 wide
    (460, 260, 132, 1),    # 128x128 / 256x256                  two row tiles (last of 204) x two column tiles (last 4 wide)
    (768, 224, 252, 3),    # 128x128 / 256x256                  three full row tiles, N tail, K ends inside a slab
    (460, 224, 256, 9),    # 128x128 / 256x256                  whole slabs, one XCD round of maps plus one
]


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("R,C,NP,S", ONE_CHUNK)
def test_tile_edges_in_one_chunk(L, mode, R, C, NP, S):
    """M, N and K tails of every k-contiguous-B instance: one slab per map, 1 / 3 / 9 maps (9 = one round over the 8 XCDs of
    the work-group order plus one item)."""
    L.check(L.lib().csn_set_math_mode(mode))
    assert _slabs(L, R, C, S, NP)[1] == 1
    a, b, G, T = _operands(S, R, C, NP)
    _check(_wgrad(L, a, b, R, C, NP), G, T, mode, what=f"{R}x{C}x{NP}x{S}")


# ---- 2. several chunks ---------------------------------------------------------------------------------------------------------
# n_maps, n_points, chunks per map, rows, channels
CHUNKED = [
    (1, 260, 2, 36, 100),         # 132 + 128 points                  64 x 128 instance
    (3, 1000, 4, 768, 256),       # 252 x 3 + 244                     256 x 256 (mode 0: 128 x 128), the largest case of this module
    (2, 1300, 6, 200, 132),       # 220 x 5 + 200                     128 x 128, M tail of 72 and a column tile 4 wide
]


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("S,NP,chunks,R,C", CHUNKED)
def test_several_chunks_fill_every_slab(L, mode, S, NP, chunks, R, C):
    """Equal chunks with a shorter last one.  The slab count is what csn_wgrad_workspace_floats implies; the workspace has exactly
    that many floats and starts as NaN, so a dw without NaN means every element of every slab was written, and the guards behind
    workspace and dw mean nothing else was.  The last chunk's points end 8 / 24 columns before the row does: reading a full
    chunk there (no clamp to the points left) meets NaN."""
    L.check(L.lib().csn_set_math_mode(mode))
    assert _slabs(L, R, C, S, NP)[1] == chunks
    a, b, G, T = _operands(S, R, C, NP)
    got = _wgrad(L, a, b, R, C, NP, pad_a=8, pad_x=24)
    _check(got, G, T, mode, elementwise=True, what=f"{S} maps of {NP} points")


# ---- 3. pitches and strides ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("R,C,NP,S,pad_a,pad_x", [(72, 100, 260, 3, 12, 4), (200, 260, 236, 2, 4, 20), (36, 36, 132, 4, 8, 28)])
def test_row_pitches_and_shape_strides(L, mode, R, C, NP, S, pad_a, pad_x):
    """ld_dout != ld_x, both above n_points, and shape strides of twice the map size (the slots in between are NaN): the
    x[::2] form of test_gpu_wx.test_strided_slots_and_an_output_that_ends_its_allocation, for both maps."""
    L.check(L.lib().csn_set_math_mode(mode))
    a, b, G, T = _operands(S, R, C, NP)
    got = _wgrad(L, a, b, R, C, NP, pad_a=pad_a, pad_x=pad_x, step=2)
    _check(got, G, T, mode, elementwise=_slabs(L, R, C, S, NP)[1] > 1, what=f"pitches {NP + pad_a}/{NP + pad_x}, every second slot")


# ---- 4. accumulate and scale ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("R,C,NP,S", [(36, 100, 132, 3), (200, 224, 260, 2), (96, 132, 1000, 1)])
def test_accumulate_adds_the_scaled_new_term(L, mode, R, C, NP, S):
    """accumulate = 1, scale = 0.5 on a dw that holds P: P + 0.5 G (the scale applies to the new term only, not 0.5 (P + G)), and
    after two more calls P + 1.5 G.  P is as large as G, so either mistake is O(1) relative."""
    L.check(L.lib().csn_set_math_mode(mode))
    a, b, G, T = _operands(S, R, C, NP)
    rng = np.random.default_rng(41)
    P = torch.from_numpy((rng.standard_normal(size=(R, C)) * math.sqrt(S * NP)).astype(np.float32))
    once = _wgrad(L, a, b, R, C, NP, scale=0.5, accumulate=1, prefill=P)
    _check(once, P.double() + 0.5 * G, T, mode, what="P + 0.5 G")
    thrice = _wgrad(L, a, b, R, C, NP, scale=0.5, accumulate=1, prefill=P, calls=3)
    _check(thrice, P.double() + 1.5 * G, T, mode, what="P + 1.5 G")


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("D,C", [(32, 36), (96, 100)])
def test_ranged_plans_accumulate_row_groups_of_one_pool(L, mode, D, C):
    """The ranged form of the attention backward (csn_amd/functional.py, "projection weight gradients"): one (S, 3 D, NP)
    gradient tensor, the row groups [0, D) and [D, 3 D), each contracted over two slot ranges (first, step, count) — the first
    with accumulate = 0, the second with 1 — from a pointer offset into both maps, into dw carved at rows0 * C of one (3 D, C)
    pool.  Equal to the float64 gradient of the whole tensor; a group's calls leave the other group's rows bit for bit alone.
    Row counts 32 / 64 (the 64 x 128 instance up to its limit) and 96 / 192 (128 x 128, one and two row tiles)."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(mode))
    S, NP, ld = 5, 260, 264
    a, b, G, T = _operands(S, 3 * D, C, NP)
    host_a = torch.full((S, 3 * D, ld), NAN)
    host_a[:, :, :NP] = a
    host_x = torch.full((S, C, ld), NAN)
    host_x[:, :, :NP] = b
    _, ad, a_front, a_back = _carve(host_a.numel(), front=GUARD)
    _, xd, x_front, x_back = _carve(host_x.numel(), front=GUARD)
    ad.copy_(host_a.reshape(-1))
    xd.copy_(host_x.reshape(-1))
    _, dw, dw_front, dw_back = _carve(3 * D * C, front=GUARD)
    dwv = dw.view(3 * D, C)
    groups = ((0, D, ((0, 2, 3), (1, 2, 2))), (D, 2 * D, ((0, 1, 2), (2, 1, 3))))       # every slot once per group
    for rows0, nrows, ranges in groups:
        before = dwv.clone()
        for i, (first, step, count) in enumerate(ranges):
            ws_n, _ = _slabs(L, nrows, C, count, NP)
            _, ws, _, ws_guard = _carve(ws_n)
            L.check(lib.csn_project_wgrad_f32(ad.data_ptr() + 4 * (first * 3 * D + rows0) * ld, step * 3 * D * ld, ld,
                                              xd.data_ptr() + 4 * first * C * ld, step * C * ld, ld,
                                              dw.data_ptr() + 4 * rows0 * C, nrows, C, count, NP, 1.0, 0 if i == 0 else 1,
                                              ws.data_ptr(), ws_n, _stream()), "csn_project_wgrad_f32")
            torch.cuda.synchronize()
            assert torch.isnan(ws_guard).all()
        outside = torch.ones(3 * D, dtype=torch.bool, device="cuda")
        outside[rows0:rows0 + nrows] = False
        same = (dwv[outside] == before[outside]) | (torch.isnan(dwv[outside]) & torch.isnan(before[outside]))
        assert bool(same.all()), f"rows outside [{rows0}, {rows0 + nrows}) changed"
        if rows0 == 0:
            assert torch.isnan(dwv[D:]).all()                       # the second group's rows: not yet written by anyone
    for g in (a_front, a_back, x_front, x_back, dw_front, dw_back):
        assert torch.isnan(g).all()
    _check(dwv.cpu(), G, T, mode, elementwise=True, what=f"ranged, D = {D}")


# ---- 5. forms of the 256 x 256 product with k-contiguous B ---------------------------------------------------------------------
@pytest.mark.parametrize("R,C,NP,S", [(200, 260, 236, 3), (460, 224, 1000, 2)])
def test_forms_of_the_big_tile_with_k_contiguous_b(L, R, C, NP, S):
    """Mode 1.  CSN_DEV_WIDE_FORMS 7 against 3: the 16-wave against the 8-wave 256 x 256 kernel.  Both walk the same 32-point
    slabs and issue, per accumulator element, the same three bf16 products per 16-point step in the same order (lo x hi, hi x lo,
    hi x hi); the slabs are reduced by the same kernel: the design promises the same bits (gemm_bf16x3.hip, "gradients bit for bit
    those of the 8-wave kernel"), and they are asserted — for dw and for every slab of the workspace.  CSN_DEV_BIG_TILES 1 against
    0 (256 x 256 against 128 x 128): the same slabs too, but nothing promises it; both are held to the float64 tolerance."""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(1))
    a, b, G, T = _operands(S, R, C, NP)
    multi = _slabs(L, R, C, S, NP)[1] > 1
    res = {}
    for name, key, val in (("16 waves", L.DEV_WIDE_FORMS, 7), ("8 waves", L.DEV_WIDE_FORMS, 3), ("128 x 128", L.DEV_BIG_TILES, 0)):
        prev = lib.csn_dev_set(key, val)
        try:
            res[name] = _wgrad(L, a, b, R, C, NP, keep_ws=True)
        finally:
            lib.csn_dev_set(key, prev)
        _check(res[name][0], G, T, 1, elementwise=multi, what=name)
    assert torch.equal(res["16 waves"][1], res["8 waves"][1])         # every slab ...
    assert torch.equal(res["16 waves"][0], res["8 waves"][0])         # ... and the gradient: bit for bit
    _check(res["128 x 128"][0], res["16 waves"][0].double(), T, 1, what="big against small tiles")


# ---- 6. the out-projection's dW ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fp32", "bf16x3", "bf16x3-tiled"])
@pytest.mark.parametrize("C,D,NP,E", [(32, 64, 36, 1), (96, 192, 132, 3), (256, 256, 260, 2)])
def test_out_projection_weight_gradient_accumulates(L, route, C, D, NP, E):
    """csn_outproj_ln_bwd_f32 with accumulate = 1 on a dwfc that holds P: P + sum_{e,n} dz[e][c][n] ctx[e][D][n], the float64
    product taken from the dz the call itself returns — the product alone, whatever the LayerNorm backward does (it has its
    own tests).  Mode 0, mode 1 as routed by default (256 x 256: dCtx on the streaming kernel) and with CSN_DEV_WX = 0.  ctx is
    read by the weight gradient only: its pad columns are NaN; dz starts as NaN, so are its pad columns unless written."""
    lib = L.lib()
    mode = 0 if route == "fp32" else 1
    L.check(lib.csn_set_math_mode(mode))
    if route == "bf16x3-tiled":
        lib.csn_dev_set(L.DEV_WX, 0)
    rng = np.random.default_rng(100 * C + E)
    ld = NP + 4
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(size=s).astype(np.float32))
    zpad = lambda t: torch.nn.functional.pad(t, (0, ld - NP))
    dxhat, xhat = zpad(rnd(E, C, NP)).cuda(), zpad(rnd(E, C, NP)).cuda()
    rstd = (torch.from_numpy(rng.random(size=(E, NP)).astype(np.float32)) + 0.5).cuda()
    ctx_h = rnd(E, D, NP)
    _, ctx, ctx_guard = _padded(ctx_h, ld)
    wfc_t = (rnd(D, C) / math.sqrt(C)).cuda()
    P = rnd(C, D) * math.sqrt(E * NP)
    _, dz, _, dz_guard = _carve(E * C * ld)
    _, dctx, _, dctx_guard = _carve(E * D * ld)
    _, dw, _, dw_guard = _carve(C * D)
    dw.copy_(P.reshape(-1))
    ws_n, _ = _slabs(L, C, D, E, NP)
    _, ws, _, ws_guard = _carve(ws_n)
    L.check(lib.csn_outproj_ln_bwd_f32(dxhat.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), C * ld, ctx.data_ptr(), D * ld,
                                       wfc_t.data_ptr(), dz.data_ptr(), None, dctx.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws_n,
                                       E, C, D, ld, NP, 1, 0.0, 0, 0, 0, None, E, None, 1, _stream()), "csn_outproj_ln_bwd_f32")
    torch.cuda.synchronize()
    for g in (ctx_guard, dz_guard, dctx_guard, dw_guard, ws_guard):
        assert torch.isnan(g).all()
    dz_h = dz.view(E, C, ld)[:, :, :NP].cpu().double()
    assert not torch.isnan(dz_h).any()
    G = torch.einsum("ecn,edn->cd", dz_h, ctx_h.double())
    T = torch.einsum("ecn,edn->cd", dz_h.abs(), ctx_h.double().abs())
    _check(dw.view(C, D).cpu(), P.double() + G, T, mode, what=f"dwfc {C}x{D}, {E} evaluations of {NP}")


# ---- 7. the single-product modes with fp32 maps --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 3], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S,NP,R,C", [(s, n, r, c) for s, n, _, r, c in CHUNKED] + [(3, 12, 36, 100), (3, 4, 200, 260)])
def test_single_product_modes_against_rounded_operands(L, mode, S, NP, R, C):
    """Modes 2 / 3 round every operand once to bf16 / fp16 and are outside the 1e-4 contract (test_gpu_lowprec.py), so they are
    not held to float64 of the fp32 operands.  The reference is the float64 product of the operands rounded to the mode's type
    (round to nearest even on both sides: csn_mode::to16x4 is a plain fp32 -> 16-bit conversion): products of two 16-bit numbers
    are exact in fp32, so what remains is fp32 accumulation and the mode-0 tolerance applies — a dropped chunk or a misread
    point is O(1) against it.  The multi-chunk shapes of case 2 and two one-chunk shapes (64 x 128 and the 8-wave 256 x 256)."""
    L.check(L.lib().csn_set_math_mode(mode))
    a, b, G, T = _operands(S, R, C, NP, rounded=mode)
    multi = _slabs(L, R, C, S, NP)[1] > 1
    got = _wgrad(L, a, b, R, C, NP, pad_a=8, pad_x=24)
    _check(got, G, T, mode, elementwise=multi, what=f"{R}x{C}, {S} maps of {NP}")


# ---- 8. reproducibility --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
def test_two_calls_give_the_same_bits(L, mode):
    """The slabs are added in a fixed order by one thread per four elements: two identical calls, the same bits."""
    L.check(L.lib().csn_set_math_mode(mode))
    S, NP, _, R, C = CHUNKED[2]
    a, b, _, _ = _operands(S, R, C, NP)
    first, second = _wgrad(L, a, b, R, C, NP), _wgrad(L, a, b, R, C, NP)
    assert not torch.isnan(first).any() and torch.equal(first, second)


# ---- 9. channels that are not a multiple of 4 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["fp32", "bf16x3", "bf16", "fp16"])
def test_channels_off_a_multiple_of_four_are_refused_before_any_launch(L, mode):
    """channels is the N of the product and the row pitch of every slab; the epilogues and the slab reducer move 16-byte chunks.
    CSN_E_ALIGN in every math mode, and nothing was launched: dw and the workspace are still NaN.  (With this refusal no entry
    point reaches the slab reducer with n % 4 != 0: rows_fc and sparse_conv take channel counts that are multiples of 32.)"""
    lib = L.lib()
    L.check(lib.csn_set_math_mode(mode))
    S, R, C, NP = 2, 64, 62, 40
    dout, x = torch.zeros(S, R, NP, device="cuda"), torch.zeros(S, 64, NP, device="cuda")
    ws_n = lib.csn_wgrad_workspace_floats(R, 64, S, NP)
    _, ws, _, _ = _carve(ws_n)
    _, dw, _, _ = _carve(R * 64)
    for acc in (0, 1):
        rc = lib.csn_project_wgrad_f32(dout.data_ptr(), R * NP, NP, x.data_ptr(), 64 * NP, NP, dw.data_ptr(), R, C, S, NP, 1.0, acc,
                                       ws.data_ptr(), ws_n, _stream())
        assert rc == ALIGN
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(ws).all()
