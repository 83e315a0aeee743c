/* csn_hip.h — C ABI of libcsn_hip.so: the MI355X (gfx950) implementation of CSN's cross-shape-attention
 * hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 * `stream` is a hipStream_t passed as void*.  All functions return 0 on success, a negative CSN_E_* code
 * on a rejected argument, or a positive hipError_t from the launch.  Nothing here allocates, synchronises
 * or touches the host: every entry point only enqueues kernels on `stream` (graph-capture safe).
 *
 * The reference (marios2019/CSN) has no native layer at all: its hot path is the PyTorch op sequence in
 * MID-FC/csa_models.py.  Each entry point below names the reference lines whose arithmetic it replaces;
 * the Python binding that a maintainer of the reference would add is shown in INTEGRATION.md and lives
 * in csn_amd/_lib.py.
 *
 * DATA LAYOUT.  Every activation is CHANNEL-MAJOR fp32: a per-shape feature map is [channels][points]
 * with leading dimension `ld` (>= points) — exactly the reference's (B, C, N, 1) input
 * (MID-FC/features_data_loader.py:45-48, csa_models.py:88-94).  "shape slot" = one 3D shape's feature map;
 * "evaluation" = one multi-head-attention call MHA(x_q; x_kv) of csa_models.py:81-125 (a CSA forward of
 * one query shape with K neighbours is 2K+1 distinct evaluations, csa_models.py:209-242).
 * Points are processed in `n_blocks` consecutive blocks of `block` points; query block i attends to
 * key/value block i only (csa_models.py:83-90: 20 blocks of 500).
 * Alignment contract (checked, CSN_E_ALIGN): device pointers 16-byte aligned; ld, block, n_points,
 * channel counts and all strides multiples of 4 floats; head dim in {32,64,96,128,256};
 * d_model in {32,64,96,128,256}.
 */
#ifndef CSN_HIP_H
#define CSN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CSN_ABI_VERSION 17
/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY exported symbols. */
#define CSN_API __attribute__((visibility("default")))

/* math modes (csn_set_math_mode / csn_set_thread_math_mode) */
#define CSN_MATH_FP32 0
#define CSN_MATH_BF16X3 1
#define CSN_MATH_BF16 2
#define CSN_MATH_FP16 3

#define CSN_E_ARG (-1)     /* null pointer / non-positive size / a count beyond its row (leading dimension) / bad flag */
#define CSN_E_ALIGN (-2)   /* a size or leading dimension is not % 4      */
#define CSN_E_PTR (-3)     /* pointer not 16-byte aligned                  */
#define CSN_E_STRIDE (-4)  /* a stride is not % 4                          */
#define CSN_E_DIM (-5)     /* unsupported head / model dimension           */
#define CSN_E_WORKSPACE (-6) /* workspace too small                        */

/* ABI version of the loaded library (== CSN_ABI_VERSION). */
CSN_API int csn_version(void);
/* Arithmetic of the contractions (projections, attention products, out-projection, every gradient product):
 *   0 CSN_MATH_FP32    exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4: bit-identical to an fmaf chain);
 *   1 CSN_MATH_BF16X3  every fp32 operand is split into two bf16 terms and a product is three bf16 MFMAs
 *                      (hi*hi + hi*lo + lo*hi, fp32 accumulate): ~1e-5 relative error per product, 5.3x the fp32 matrix rate.
 *                      THE DEFAULT: like mode 0 it is inside the 1e-4 contract of the path (every parity test runs in both);
 *   2 CSN_MATH_BF16    every operand rounded once to bf16, one MFMA per product, fp32 accumulate; tile planes hold one
 *                      plane (half the bytes).  OUTSIDE the 1e-4 contract: ~1e-2 relative on outputs (reported by the tests);
 *   3 CSN_MATH_FP16    the same with fp16 operands — FORWARD entry points only (gradients of this path reach 1e-7 and
 *                      underflow fp16): the backward entry points return CSN_E_ARG in this mode; callers run them in mode 2
 *                      (csn_amd does: "fp16 forward / bf16 backward").
 * The retrieval measure (7) always runs in exact fp32 (bit-exact kNN indices); the fp16 screen of (11b) never decides a rank: it
 * only names candidates that provably cannot be ranked, and every candidate it keeps is scored in fp32.
 * The cross-length entry points (3b) have no single-product kernels: in modes 2 / 3 they run as mode 1.
 * The row products of the MinkowskiNet side — (13) csn_rows_fc_*, (14) csn_sparse_conv_*, (15a) csn_sparse_conv_stats_fwd_f32 —
 * have single-product instances behind a per-thread, opt-in flag, csn_set_thread_rows16(on): on = 0 (THE DEFAULT) runs modes 2 / 3
 * as mode 1 there, as before the instances existed; on = 1 runs mode 2 in every forward and backward entry point of those sections
 * (the folded eval epilogue of csn_rows_fc_fwd_f32 included) and mode 3 in their FORWARD entry points (csn_sparse_conv_fwd_f32,
 * csn_sparse_conv_stats_fwd_f32, csn_rows_fc_fwd_f32) with every operand rounded once to 16 bits (nearest even), one
 * v_mfma_f32_32x32x16_{bf16,f16} per product, fp32 accumulation, fp32 maps in memory as ever; mode 3 then makes
 * csn_sparse_conv_bwd_f32 and csn_rows_fc_bwd_f32 return CSN_E_ARG before any launch (callers run them in mode 2).  Modes 0 and 1
 * do not see the flag.  Any other value of `on` returns CSN_E_ARG and leaves the flag; csn_get_thread_rows16 returns it.
 * What the matrix instruction does with fp16 SUBNORMAL operands (|v| < 2^-14) is not pinned.
 * csn_set_math_mode sets the PROCESS default; csn_set_thread_math_mode overrides it for the calling thread only (-1 clears the
 * override), which is how a module selects its own mode per call without touching other threads (csn_amd brackets every
 * forward / backward with it; autograd's backward threads set their own).  csn_get_math_mode returns the mode in effect for
 * the calling thread.  Both setters return CSN_E_ARG for an unknown value. */
/* SPLIT TENSORS (math mode 1).  Arguments named *_split / *_plane_stride let a kernel write, or read, an fp32
 * tensor as two bf16 planes x = hi + lo (hi = bf16(x), lo = bf16(x - hi)): the pointer then addresses the HIGH
 * plane (bf16 elements, cast to float* for the ABI), the LOW plane starts `plane_stride` bf16 elements later, and
 * every stride / leading dimension of that tensor counts bf16 elements (same numbers as for the fp32 tensor).
 * The producer's epilogue splits once; consumers stage the planes into LDS with plain copies (no conversion work per
 * tile).  A split dctx (attention-output gradient) is laid out [evaluation][2 planes][n_heads*d_head][ld]: its
 * evaluation stride is 2 * ctx_eval_stride and dctx_plane_stride = ctx_eval_stride.
 * TILE PLANES (math modes 1..3): the form in which keys and values travel from the projection to the attention kernels
 * (described for mode 1, two planes; in modes 2 / 3 there is ONE plane of bf16 / fp16 elements: a tile is [32 keys], the block
 * pitch 512, ld_out = n_blocks * 512, and a probs_tiles backward leaves P and dS as compact rows — see (3)).
 * csn_project_f32 with out_split = 2 writes, per output row and per attention block of `out_plane_stride` (<= 512) points,
 * 16 tiles of [hi: 32 keys | lo: 32 keys] bf16 — block pitch 1024, row pitch ld_out = n_blocks * 1024, out_shape_stride in
 * bf16 elements; the padding keys of a block's last 32-key tile are written as zeros (tiles beyond it are not touched and never read).  Every 32-key tile row is then
 * 128 contiguous, 128-byte aligned bytes that the attention kernels stage into LDS with plain copies.  The attention
 * entry points take such a tensor for k and v when qkv_split / kv_split != 0 (then *_plane_stride = that row pitch and
 * kv_shape_stride counts bf16 elements); q stays fp32.
 * STATUS: live are csn_project_f32 out_split (1: whole planes, 2: tile planes), csn_outproj_ln_bwd_f32 dctx_split, and the
 * k/v tile planes of csn_block_attn_fwd_f32 / csn_block_attn_bwd_dq_f32; dctx_split / q_split INPUTS are reserved
 * (CSN_E_ARG).  Passing *_split != 0 in math mode 0 returns CSN_E_ARG. */
/* 16-BIT ACTIVATION MAPS (math modes 2 and 3).  In the single-product modes every matrix operand is rounded to 16 bits when it
 * is staged, so the maps the entry points hand to each other can travel in that form: half the bytes, and the consumers stage
 * them by copy.  csn_set_thread_act16(fmt) switches the CALLING THREAD's calls to that exchange format — fmt 1: the forward's
 * maps are bf16 (a math-mode-2 forward), fmt 2: they are fp16 (a math-mode-3 forward; its backward runs in mode 2 and converts
 * them in registers while staging), 0: off (the default: everything below is fp32).  With the flag set
 *   Qs   (csn_project_f32 out_split = 3 writes it; read by (2), by the recomputing calls of (3) and by the dK product)   fwd type
 *   Ctx  (written by (2); read by (4) forward, by (3)'s delta and by the W_fc gradient of (4) backward)                 fwd type
 *   xhat (written by (4) forward; read by (4) backward and by (6))                                                      fp16 always (|xhat| < sqrt(C))
 *   dZ, dCtx (written by (4) backward; read by (3))                                                                     bf16
 *   dQ, dK, dV (fmt + 4 only: written by (3), read by csn_project_wgrad_f32 and, as x, by csn_project_f32 out_split + 16)    bf16
 * are ONE plane of 16-bit elements with the shapes documented below; their pointers stay typed float* and every stride and
 * leading dimension of such a map counts 16-bit ELEMENTS (same numbers as for the fp32 map).  Everything else keeps its type:
 * the input maps x, the residual, dxhat / dfeats, lse / delta / rstd, every gradient map dQ / dK / dV / dz_res, weights and
 * weight gradients, the K / V tile planes (already 16-bit).  Products are bit-identical to the fp32 exchange wherever a map is
 * only a matrix operand (it was rounded to the same 16 bits at staging) and a 16-bit output map holds the fp32 map's values
 * rounded once — both held bit for bit by tests/test_gpu_act16_edges.py; delta = sum dO * O, the LayerNorm backward and the mix
 * see the rounded maps (|xhat| error <= 2^-11 relative).  Requirements: math mode 2 / 3 with K / V tile planes, block mode (no
 * cross-length entry points), no split tensors, a mix backward without gradient maps (the linked form), evaluation outputs
 * written once (no accumulate into a 16-bit map).  A forward entry point returns CSN_E_ARG when fmt does not name its mode's
 * type; backward entry points take either fmt in mode 2.  fmt + 4 (5 or 6) also makes the gradient maps dQ / dK / dV bf16:
 * they are then written once per slot (grouped calls; accumulate != 0 returns CSN_E_ARG), and what contracts them rounds them to
 * bf16 anyway — the weight gradients are the same bits. */
CSN_API int csn_set_thread_act16(int fmt);
CSN_API int csn_get_thread_act16(void);
/* single-product row products of (13), (14), (15a) for the calling thread: see the math-mode comment above */
CSN_API int csn_set_thread_rows16(int on);
CSN_API int csn_get_thread_rows16(void);
/* SCORE STORAGE of the block-attention entry points (3), (3c), per calling thread.  0 (default): the scores of a block are
 * [query][key] rows of pitch score_pitch — what a caller that reads probabilities expects.  1: TILE-MAJOR — per block
 * [key tile of 32][query][32 keys]: the forward's scores, and the P / dS tile planes the backward hands from its dQ call to its
 * dK / dV call, are then written and read in contiguous runs (a wave instruction moves 1 KB in one piece instead of sixteen
 * 64-byte pieces 2 KB apart).  Same arithmetic, same buffer sizes; only meaningful when the three calls of one evaluation batch
 * agree.  Taken where csn_attn_bwd_grouping reports bit 4 (bf16x3 mode, block mode, tile-plane K / V, probs_tiles = 1, the dK / dV
 * products on the 256 x 256 tiles); CSN_E_ARG otherwise.  csn_amd sets it around the training step's three calls. */
CSN_API int csn_set_thread_score_layout(int layout);
CSN_API int csn_get_thread_score_layout(void);
CSN_API int csn_set_math_mode(int mode);
CSN_API int csn_set_thread_math_mode(int mode);
CSN_API int csn_get_math_mode(void);
/* The calling thread's own override as set by csn_set_thread_math_mode (-1 = none): what a scoped override saves and restores. */
CSN_API int csn_get_thread_math_mode(void);
/* Human-readable text for a status code returned by any function below. Host pointer, static storage. */
CSN_API const char* csn_status_string(int status);

/* ---- (1) pre-attention projections ------------------------------------------------------------------
 * out[s][r][n] = sum_c w[r][c] * x[s][c][n],  r < rows, n < n_points; rows r < div_rows are then divided
 * by `temperature`.   Replaces w_qs / w_ks / w_vs (nn.Linear, no bias; csa_models.py:49-51,103-105) and the
 * `q / temperature` of csa_models.py:139 (stack W_q|W_k|W_v along rows and pass div_rows = n_head*d_k to
 * project a shape once for all of its evaluations).  out_split: 0 fp32 maps, 1 / 2 split tensors / tile planes (above), 3 (math
 * modes 2 / 3): ONE 16-bit map per shape in the mode's type — out_shape_stride and ld_out count 16-bit elements.  out_split + 16
 * (math mode 2): x itself is a bf16 map (x_shape_stride, ld_x in elements) — the input gradient W^T dqkv from bf16 gradient maps. */
CSN_API int csn_project_f32(const float* x, long long x_shape_stride, int ld_x, const float* w, int rows, int channels,
                    float* out, long long out_shape_stride, int ld_out, int n_shapes, int n_points, int div_rows,
                    float temperature, int out_split, long long out_plane_stride, void* stream);

/* Q, K and V of the same slots in one call (csa_models.py:103-105 on one input): w_qkv = [W_q ; W_k ; W_v] (3 d_inner rows),
 * Qs = W_q x / temperature as an fp32 map q_out [slot][d_inner][ld_q], K | V as tile planes kv_out [slot][2 d_inner][ld_kv] —
 * exactly what csn_project_f32(.., div_rows = d_inner, out_split = 0) and csn_project_f32(.., out_split = 2,
 * out_plane_stride = block) write, bit for bit; 16-bit math modes only (tile planes).  In the bf16x3 mode with 256 channels and
 * d_inner = 256 the three row sets share ONE pass over x (the streaming kernel); elsewhere it is the two calls. */
CSN_API int csn_project_qkv_f32(const float* x, long long x_shape_stride, int ld_x, const float* w_qkv, int d_inner, int channels,
                        float* q_out, long long q_shape_stride, int ld_q, void* kv_out, long long kv_shape_stride, int ld_kv,
                        int n_shapes, int n_points, float temperature, int block, void* stream);

/* ---- (1b) folded projections: W_k folded into W_q, W_v into W_fc (one head, d_head = d_model, no biases) -------------------
 * With one head, bias-free linear layers and nothing non-linear between a projection and the product that consumes it, the
 * scores and the out-projection re-associate (row-per-point notation, t = the temperature):
 *   S = (x_q W_q^T / t)(x_k W_k^T)^T = (x_q M^T) x_k^T,     M    = W_k^T W_q / t     [channels][channels]
 *   fc(P (x_k W_v^T))                = (P x_k) W_fv^T,      W_fv = W_fc W_v          [channels][channels]
 * so the attention calls of (2) and (3) run on the INPUT's tile planes as both K and V, and K, V, dK and dV never exist.
 * csn_fold_weights_f32: m, w_fv and w_fv_t (= W_fv^T, which (5) / (5b) stream) from w_q, w_k, w_v [d_inner][channels] and w_fc
 *   [channels][d_inner].  csn_unfold_wgrads_f32: from dm = dLoss/dM and dw_fv = dLoss/dW_fv
 *   dw_q = W_k dM / t,  dw_k = W_q dM^T / t,  dw_fc = dW_fv W_v^T,  dw_v = W_fc^T dW_fv.
 * Both run exact fp32 products (the fp32 matrix-core GEMM) WHATEVER the thread's math mode, and divide by t as a true division.
 * ws: csn_fold_workspace_floats(d_inner, channels) floats for the fold, d_inner * channels for the unfold (transposed weights).
 * csn_tile_planes_f32: x [shape][rows][ld_x] fp32 -> the bf16 tile planes csn_project_f32 writes with out_split = 2 in math mode 1
 *   (per row and block of `block` points 16 tiles of [hi 32 | lo 32], hi = bf16(x), lo = bf16(x - hi); ld_out = row pitch, a
 *   multiple of 1024 and >= n_blocks * 1024; out_shape_stride in 16-bit elements) — a copy with a split, no product: the layout
 *   and (to the last bit of lo) the values of that projection with an identity weight.  The padding keys of every block's last tile are written as zeros, the tiles beyond a
 *   short last block are not written (nothing reads them).  Mode-independent (the layout is math mode 1's). */
CSN_API long long csn_fold_workspace_floats(int d_inner, int channels);
CSN_API int csn_fold_weights_f32(const float* w_q, const float* w_k, const float* w_v, const float* w_fc, int d_inner, int channels,
                                 float temperature, float* m, float* w_fv, float* w_fv_t, float* ws, long long ws_floats,
                                 void* stream);
CSN_API int csn_unfold_wgrads_f32(const float* dm, const float* dw_fv, const float* w_q, const float* w_k, const float* w_v,
                                  const float* w_fc, int d_inner, int channels, float temperature, float* dw_q, float* dw_k,
                                  float* dw_v, float* dw_fc, float* ws, long long ws_floats, void* stream);
CSN_API int csn_tile_planes_f32(const float* x, long long x_shape_stride, int ld_x, void* out, long long out_shape_stride,
                                int ld_out, int n_shapes, int rows, int n_points, int block, void* stream);

/* ---- (2) block-diagonal scaled-dot-product attention, forward ----------------------------------------
 * For evaluation e, head h, block b:  P = softmax(Qs K^T) over the block's keys, ctx = P V
 * (ScaledDotProductAttention.forward, csa_models.py:138-144, eval mode; Qs is already divided by the
 * temperature by csn_project_f32).  q/k/v point at row 0 of the projected [n_heads*d_head][ld] maps of
 * slot 0; evaluation e reads slot q_index[e] (queries) and kv_index[e] (keys, values); NULL = identity.
 *   ctx    [n_evals][n_heads*d_head][ld]   (eval stride given)         — csa_models.py:114 before `fc`
 *   lse    [n_evals][n_heads][n_blocks*block]   log-sum-exp of every score row (for the backward); may be NULL (inference)
 *   scores [n_evals][n_heads][n_blocks][block][score_pitch]  raw scores S[query][key]; may be NULL
 *          (inference).  score_pitch >= block, % 4.
 * RAGGED LAST BLOCK: when n_blocks * block > ld the row of ld points ends inside the last block, which then holds
 * ld - (n_blocks - 1) * block points (a multiple of 4; CSN_E_ARG if that is not positive): queries and keys of the last block
 * are cut there in all three block-attention entry points.  lse / delta / scores keep their n_blocks * block layout.
 * rescale_threshold: the running softmax maximum is only re-based when it grows by more than this
 * (0 = re-base on every key tile); results agree to fp32 rounding for any value <= ~40.
 * dropout_p / seed: train-mode dropout on the probabilities (nn.Dropout(0.1), csa_models.py:133-141):
 * P_drop = mask * P / (1 - p) with a counter-based mask, a pure function of (seed, position in `scores`), so
 * the backward call regenerates it from the same (dropout_p, seed).  0 = eval mode. */
CSN_API int csn_block_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                           long long kv_shape_stride, const int* q_index, const int* kv_index, int ld, float* ctx,
                           long long ctx_eval_stride, float* scores, float* lse, int n_evals, int n_heads,
                           int d_head, int block, int n_blocks, int score_pitch, float rescale_threshold,
                           float dropout_p, unsigned long long seed, int qkv_split, long long qkv_plane_stride,
                           void* stream);

/* The same forward with the evaluations GROUPED BY QUERY SLOT: group g = eval_ids[group_offsets[g] .. group_offsets[g+1])
 * (device int32 arrays; every evaluation of [0, n_evals) listed exactly once; all evaluations of a group have the same
 * q_index — CSN_E_ARG semantics are the caller's: the library does not read the arrays on the host).  In the 16-bit math modes a
 * work-group stages the pre-scaled queries of its 128-query tile ONCE and runs the group's evaluations one after the other
 * with the operand in registers (the query shape of a CSA step serves K+2 evaluations: csa_models.py:210, 232-237 — half of
 * the step's operand blocks are never fetched); in the fp32 mode the evaluations run ungrouped.  Every output is the
 * ungrouped call's, bit for bit. */
CSN_API int csn_block_attn_fwd_grouped_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                           long long kv_shape_stride, const int* q_index, const int* kv_index, int ld, float* ctx,
                           long long ctx_eval_stride, float* scores, float* lse, int n_evals, int n_heads,
                           int d_head, int block, int n_blocks, int score_pitch, float rescale_threshold,
                           float dropout_p, unsigned long long seed, int qkv_split, long long qkv_plane_stride,
                           const int* eval_ids, const int* group_offsets, int n_groups, void* stream);

/* ---- (3) block attention, backward (autograd of csa_models.py:139-142) -------------------------------
 * Two calls, because their outputs are shared differently between evaluations (the query shape's Q serves
 * K+1 evaluations, a neighbour's K/V serve two): each call processes the `n_launch_evals` evaluations listed in
 * `eval_ids` (NULL = 0..n-1) and writes into per-SLOT gradient maps, adding to them when `accumulate` != 0.  The
 * caller groups evaluations so that no two evaluations of one call share an output slot.
 *
 * csn_block_attn_bwd_dq_f32:  in  dctx, ctx [eval][n_heads*d_head][ld], k/v + kv_index as in forward,
 *                                 scores (S[query][key] from forward), lse;
 *                             out scores := P_drop (in place; = P without dropout), dscores := dS,
 *                                 delta [eval][n_heads][n_blocks*block] scratch = rowsum(dctx*ctx),
 *                                 dq[dq_index[e]] (+)= dS K   — gradient w.r.t. the pre-scaled queries Qs.
 * csn_block_attn_bwd_dkv_f32: in  dctx, q + q_index as in forward, probs (= scores after the dq call), dscores;
 *                             out dv[dv_index[e]] (+)= P^T dctx,  dk[dk_index[e]] (+)= dS^T Qs.
 * dq/dk/dv point at row 0 of the [n_heads*d_head][ld] gradient map of slot 0; *_slot_stride in floats.
 * probs_tiles != 0 (math modes 1, 2; score_pitch >= block rounded up to 32): the dq call leaves P_drop and dS as TILE
 * PLANES and the dkv call must be told the same; the dV / dK products then stage them with plain copies.  Mode 1: per query
 * row 16 tiles of [hi: 32 keys | lo: 32 keys] bf16 — the bytes of the fp32 row — P in place over `scores`, dS in `dscores`.
 * Mode 2 (one plane): rows of 16 tiles of [32 keys] are half the bytes, so both go to `dscores` — per (evaluation, head,
 * block) region of block * score_pitch floats: [P: block rows | dS: block rows] of pitch score_pitch bf16 elements — and
 * `scores` is left untouched; the dkv call reads both from its `dscores` argument (`probs` is ignored).  Mode 2 REQUIRES
 * kv_split and probs_tiles.
 * probs_tiles == 2 (csn_block_attn_bwd_dq_f32 only; mode 1, kv_split, either score layout, where
 * csn_attn_bwd_dv_scores_available says so): the dq call leaves the dS planes in `dscores` as with probs_tiles = 1 and does NOT touch `scores` — P is neither split
 * nor stored; dq, delta and the dS planes are bit for bit those of probs_tiles = 1.  dV then comes from
 * csn_block_attn_bwd_dv_scores_f32 (below), which rebuilds P from the untouched scores, and dK from a
 * csn_block_attn_bwd_dkv_f32 call with probs = NULL and dv = NULL (probs_tiles = 1): that call runs the dK product alone and
 * writes the bits the two-product call writes.
 * probs_tiles == 3 (csn_block_attn_bwd_dq_f32 only; the conditions of probs_tiles = 2, where
 * csn_attn_bwd_dq_no_planes_available says so): NOTHING score-sized is written — `scores` is read-only, `dscores` is not used and
 * may be NULL; dq and delta are bit for bit those of probs_tiles = 2.  For callers with no dK / dV products behind the call
 * (folded projections, (1b): k = v = the input's planes) — such a caller has no reader for `delta` either, which may be NULL
 * with this value alone.  probs_tiles takes the values 0 .. 3; anything else is CSN_E_ARG.
 * With k == v there (mode 1, d_head = 256) the dq call fetches every key tile once for both of its tile images instead of once
 * per image — the same bits (CSN_DEV_KV_SAME, development section).
 * GROUPED calls (group_offsets != NULL): eval_ids lists the n_launch_evals evaluations ordered so that evaluations sharing
 * an output slot are adjacent, group g = entries group_offsets[g] .. group_offsets[g+1] (n_groups + 1 offsets); a group's
 * results are accumulated in registers and its slot is written once — one call for all evaluations instead of one
 * read-modify-write pass per colour.  csn_attn_bwd_grouping() says where that is available in the current math mode:
 * bit 0 = the dq call, bit 1 = the dkv call, bit 2 = csn_block_attn_bwd_dq_recompute_f32, bit 3 =
 * csn_block_attn_bwd_dkv_flash_f32 (both below), bit 4 = tile-major score storage (csn_set_thread_score_layout).
 * csn_attn_bwd_dv_scores_available() != 0: csn_block_attn_bwd_dv_scores_f32 and probs_tiles = 2 of the dq call have an instance
 * in the current math mode (mode 1, d_head = 256, block <= 512 and % 4 == 0) — a query of its own, so that the bits above keep
 * their values.
 *
 * csn_block_attn_bwd_dq_recompute_f32 — the dq call WITHOUT saved scores ("flash" data flow; math modes 1 and 2, K / V as tile
 * planes, block mode): the forward is run with scores = NULL (only lse is kept) and this call rebuilds S = Qs K^T tile by tile
 * from the pre-scaled queries q [slot][n_heads*d_head][ld] (+ q_index, as in the forward) — one more matrix product per tile
 * against 4 * block bytes of score traffic per query in each direction.  Everything else as csn_block_attn_bwd_dq_f32.
 *   probs_tiles != 0: P_drop and dS still leave as tile planes for csn_block_attn_bwd_dkv_f32 — mode 1: P in `probs`, dS in
 *                     `dscores` (two scratch buffers of the scores' geometry); mode 2: both in `dscores`, `probs` unused;
 *   probs_tiles == 0: nothing is written besides delta and dq (`probs` / `dscores` may be NULL) — for a dK / dV pass that
 *                     recomputes the probabilities itself.
 * Available where three LDS tile images per stage fit: mode 2 at every head width, mode 1 up to d_head = 128 (bit 2 of
 * csn_attn_bwd_grouping); CSN_E_ARG elsewhere.
 * kv_f16 != 0 (math mode 2 only; also csn_block_attn_bwd_dkv_flash_f32, and kv_split = 2 of csn_block_attn_bwd_dq_f32): k and
 * v are the tile planes of a forward that ran in math mode 3 — fp16 bits.  The kernels convert every piece to bf16 in
 * registers on its way into LDS, so the "fp16 forward / bf16 backward" pairing needs no second projection of K and V. */
CSN_API int csn_attn_bwd_grouping(int d_head, int block);
CSN_API int csn_block_attn_bwd_dq_recompute_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q,
                                        long long q_shape_stride, const int* q_index, const float* k, const float* v,
                                        long long kv_shape_stride, const int* kv_index, int ld, float* probs,
                                        float* dscores, const float* lse, float* delta, float* dq,
                                        long long dq_slot_stride, const int* dq_index, int accumulate, const int* eval_ids,
                                        int n_launch_evals, int n_heads, int d_head, int block, int n_blocks,
                                        int score_pitch, float dropout_p, unsigned long long seed,
                                        long long kv_plane_stride, int kv_f16, int probs_tiles, const int* group_offsets,
                                        int n_groups, void* stream);
CSN_API int csn_block_attn_bwd_dq_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* k,
                              const float* v, long long kv_shape_stride, const int* kv_index, int ld, float* scores,
                              float* dscores, const float* lse, float* delta, float* dq, long long dq_slot_stride,
                              const int* dq_index, int accumulate, const int* eval_ids, int n_launch_evals, int n_heads,
                              int d_head, int block, int n_blocks, int score_pitch, float dropout_p,
                              unsigned long long seed, int dctx_split, long long dctx_plane_stride, int kv_split,
                              long long kv_plane_stride, int probs_tiles, const int* group_offsets, int n_groups,
                              void* stream);
CSN_API int csn_block_attn_bwd_dkv_f32(const float* dctx, long long ctx_eval_stride, const float* q, long long q_shape_stride,
                               const int* q_index, int ld, const float* probs, const float* dscores, float* dk,
                               float* dv, long long dkv_slot_stride, const int* dk_index, const int* dv_index,
                               int accumulate, const int* eval_ids, int n_launch_evals, int n_heads, int d_head,
                               int block, int n_blocks, int score_pitch, int dctx_split, long long dctx_plane_stride,
                               int q_split, long long q_plane_stride, int probs_tiles, const int* group_offsets,
                               int n_groups, void* stream);

/* csn_block_attn_bwd_dkv_flash_f32 — dK and dV WITHOUT P / dS tensors (bit 3 of csn_attn_bwd_grouping: math modes 1 and 2,
 * d_head <= 128, block mode): a work-group keeps 128 keys (256 at d_head = 96 in math mode 2 — which is also where the backward
 * of a math-mode-3 forward runs, kv_f16 = 1) of one (key/value slot, head, block)
 * in registers, streams the
 * pre-scaled queries q and the output gradient dctx of every evaluation of its group through LDS, and rebuilds P (from lse,
 * with the dropout mask of (dropout_p, seed)) and dS (with delta, as the dq call wrote it) tile by tile:
 *   dv[dv_index[e]] (+)= P_drop^T dctx,   dk[dk_index[e]] (+)= dS^T Qs
 * k / v: the tile planes of the forward (kv_plane_stride = row pitch, kv_shape_stride in 16-bit elements), kv_index as in the
 * forward; a group's evaluations must share their key and their value slot (they do when grouped by output slot).  Run after
 * csn_block_attn_bwd_dq_recompute_f32 (probs_tiles = 0), which computes delta.  eval_ids / group_offsets / accumulate as in
 * the grouped csn_block_attn_bwd_dkv_f32 call; without group_offsets every listed evaluation is its own group. */
CSN_API int csn_block_attn_bwd_dkv_flash_f32(const float* dctx, long long ctx_eval_stride, const float* q, long long q_shape_stride,
                                     const int* q_index, const float* k, const float* v, long long kv_shape_stride,
                                     const int* kv_index, long long kv_plane_stride, int kv_f16, int ld, const float* lse,
                                     const float* delta, float* dk, float* dv, long long dkv_slot_stride,
                                     const int* dk_index, const int* dv_index, int accumulate, const int* eval_ids,
                                     int n_launch_evals, int n_heads, int d_head, int block, int n_blocks, int score_pitch,
                                     float dropout_p, unsigned long long seed, const int* group_offsets, int n_groups,
                                     void* stream);

/* csn_block_attn_bwd_dv_scores_f32 — dV from the KEPT scores (where csn_attn_bwd_dv_scores_available != 0): per (value slot, head, block,
 * 128 keys) a work-group streams the forward's scores [evaluation][head][block][block][score_pitch] (fp32, in the thread's score layout, as the
 * forward wrote them — run the dq call with probs_tiles = 2), lse and dctx of every evaluation of its group, rebuilds
 * P_drop = exp(S - lse) mask / (1 - dropout_p) in registers with the mask of (dropout_p, seed), and writes
 *   dv[dv_index[e]] = P_drop^T dctx
 * once per group (no accumulate: every listed evaluation belongs to exactly one group; without group_offsets every listed
 * evaluation is its own group).  Geometry as csn_block_attn_bwd_dkv_f32 in block mode: block % 4 == 0, score_pitch >= block,
 * a row may end inside the last block (n_blocks * block > ld). */
CSN_API int csn_attn_bwd_dv_scores_available(int d_head, int block);
CSN_API int csn_attn_bwd_dq_no_planes_available(int d_head, int block);
CSN_API int csn_block_attn_bwd_dv_scores_f32(const float* dctx, long long ctx_eval_stride, int ld, const float* scores,
                                     const float* lse, float* dv, long long dkv_slot_stride, const int* dv_index,
                                     const int* eval_ids, int n_launch_evals, int n_heads, int d_head, int block, int n_blocks,
                                     int score_pitch, float dropout_p, unsigned long long seed, const int* group_offsets,
                                     int n_groups, void* stream);

/* ---- (3b) cross-length attention: one unchunked block per evaluation, n_queries != n_keys -------------
 * The MinkowskiNet variant of the layer (MinkowskiNet/models/attention.py:31-75, used per shape pair by
 * MinkowskiNet/models/hrnet.py:378-410, 456-470): softmax(Qs K^T) V over ALL keys of the other shape, gradients flowing
 * to queries, keys and values.  Same kernels as (2)/(3) with n_blocks = 1 and separate query / key counts:
 *   q, ctx, dctx, dq : [n_evals][n_heads*d_head][ld_q]   (n_queries <= ld_q)
 *   k, v, dk, dv     : [n_evals][n_heads*d_head][ld_kv]  (round-up-4(n_keys) <= ld_kv; the columns n_keys ..
 *                                                          round-up-4(n_keys) of dk / dv are written as zeros, of
 *                                                          either sign; from there to ld_kv nothing is written)
 *   scores, dscores  : [n_evals][n_heads][n_queries][score_pitch], score_pitch % 4 == 0, >= round-up-4(n_keys)
 *   lse, delta       : [n_evals][n_heads][n_queries]
 * The columns n_keys .. ld_kv of k / v must be FINITE (the last 16-byte piece of a key row is read whole and its keys beyond
 * n_keys are masked afterwards); they are never read as data.  Score rows are stored in 16-byte runs: the columns n_keys ..
 * round-up-4(n_keys) of a row may be written (-inf by the forward, 0 by the backward).
 * In math mode 1 score_pitch selects the backward's data flow: from round-up-32(n_keys) on, P_drop and dS leave the first
 * kernel as bf16 TILE PLANES (per query row tiles of [hi: 32 keys | lo: 32 keys], the bytes of the fp32 row; every tile that
 * holds a key is written, its padding keys as zeros) and the dK / dV products stage them with plain copies — what csn_amd
 * passes; below it they leave as fp32 rows (as in mode 0) and the products split them while staging.  Same results to the
 * mode's rounding; the mask pitch of the dropout is max(n_queries, score_pitch) in either flow.
 * n_keys is arbitrary; n_queries must be a multiple of 4 (pad with zero points: their rows cost little and contribute
 * nothing to any gradient).  Evaluation e reads maps e (no slot indices, no accumulation). */
CSN_API int csn_cross_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                           long long kv_shape_stride, int ld_q, int ld_kv, float* ctx, long long ctx_eval_stride,
                           float* scores, float* lse, int n_evals, int n_heads, int d_head, int n_queries, int n_keys,
                           int score_pitch, float rescale_threshold, float dropout_p, unsigned long long seed, void* stream);
CSN_API int csn_cross_attn_bwd_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                           const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                           float* scores, float* dscores, const float* lse, float* delta, float* dq, float* dk, float* dv,
                           long long dq_eval_stride, long long dkv_eval_stride, int n_evals, int n_heads, int d_head,
                           int n_queries, int n_keys, int score_pitch, float dropout_p, unsigned long long seed,
                           void* stream);

/* ---- (3c) ragged batches of the cross-length attention ("varlen") -------------------------------------------
 * ONE launch chain for a batch of shape pairs whose query and key counts all differ — MinkowskiNet/models/hrnet.py:378-410,
 * 456-470 calls the layer once per shape / per shape pair, with 1..5 k voxels each.  The entry points of (3b) with length
 * arrays: n_queries[e] and n_keys[e] are DEVICE int arrays of n_evals entries (the cu_seqlens of a padded layout); max_queries
 * (% 4) and max_keys bound them and size the grid, score_pitch and the buffers, which are PADDED to common leading dimensions:
 *   q, ctx, dctx, dq [n_evals][n_heads*d_head][ld_q],  k, v, dk, dv [n_evals][n_heads*d_head][ld_kv],
 *   scores, dscores [n_evals][n_heads][max_queries][score_pitch],  lse, delta [n_evals][n_heads][max_queries].
 * n_queries[e] % 4 == 0 (round a shape's point count up: its zero points cost little and contribute nothing); n_keys[e] is
 * arbitrary (>= 1).  Work-groups of query tiles beyond n_queries[e] exit at once and key tiles beyond n_keys[e] are never
 * visited, so a short evaluation costs its own size.  Rows / columns beyond an evaluation's own counts are neither read as
 * data nor written — with the exception (3b) has too: the dK / dV products and the score rows store 16-byte runs, so the columns
 * n_keys[e] .. round-up-4(n_keys[e]) of dk / dv are written as zeros (and those of a score row may be written).  The caller
 * zero-fills ctx, dq, dk, dv where it goes on to use the padding (csn_amd does), and the padding points of the input maps must
 * be finite (zeros).  Dropout masks are indexed with the launch's max_queries / score_pitch; the mode-1 data flow of the
 * backward is chosen by score_pitch against round-up-32(max_keys). */
CSN_API int csn_varlen_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                            long long kv_shape_stride, int ld_q, int ld_kv, float* ctx, long long ctx_eval_stride,
                            float* scores, float* lse, int n_evals, int n_heads, int d_head, int max_queries, int max_keys,
                            const int* n_queries, const int* n_keys, int score_pitch, float rescale_threshold,
                            float dropout_p, unsigned long long seed, void* stream);
CSN_API int csn_varlen_attn_bwd_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                            const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                            float* scores, float* dscores, const float* lse, float* delta, float* dq, float* dk, float* dv,
                            long long dq_eval_stride, long long dkv_eval_stride, int n_evals, int n_heads, int d_head,
                            int max_queries, int max_keys, const int* n_queries, const int* n_keys, int score_pitch,
                            float dropout_p, unsigned long long seed, void* stream);

/* ---- (3d) score-free backward of (3b) and (3c) ---------------------------------------------------------------------------
 * The backward of the cross-length and the ragged attention WITHOUT any score-sized tensor, for batches whose scores do not
 * fit the device (one score tensor is n_evals * n_heads * n_queries * score_pitch * 4 bytes; the kept flow holds three).
 * The forward runs as it does in (3b) / (3c) with scores = NULL and keeps only lse.  Then
 *   launch 1, query-stationary: rebuilds S = Qs K^T tile by tile from q and the fp32 k map (one more matrix product per
 *             tile), forms delta = rowsum(dctx * ctx) and writes delta and dq;
 *   launch 2, key-stationary:   a work-group keeps 128 keys of k and v in registers, streams q, dctx, lse and delta, rebuilds
 *             P and dS and writes dk and dv; a work-group whose keys lie beyond n_keys[e] exits at once.
 * Forward + backward cost 9 instead of 6 products of 2 * n_queries * n_keys * d_head; no P / dS is written or read.
 * Arguments: those of csn_cross_attn_bwd_f32 / csn_varlen_attn_bwd_f32 without scores and dscores; q is required, lse is
 * read, delta, dq, dk, dv are written.  Geometry, alignment and the WRITTEN REGIONS are those of (3b) / (3c): dq columns
 * < n_queries[e], dk / dv columns < round-up-4(n_keys[e]) with exact zeros in n_keys[e] .. round-up-4(n_keys[e]), delta entries
 * < n_queries[e]; nothing else.  The padding points of q, k, v, dctx, ctx, lse must be finite; delta is read back only where
 * launch 1 wrote it.  score_pitch stays an argument although no score buffer exists: the dropout mask is indexed with the pitch
 * max(n_queries, score_pitch) (max_queries for the ragged call), and both launches regenerate the forward's mask bit for bit
 * only with the forward's value (% 4, >= round-up-4(n_keys)).
 * Available in math mode 1 at d_head = 32, 64, 96, 128 (the instances of the recomputing kernels: three LDS images of two
 * planes per stage fit one CU up to d_head = 128); modes 2 and 3 run as mode 1, like (3b) / (3c).  Math mode 0 and d_head = 256
 * return CSN_E_ARG before any launch.  csn_cross_attn_flash_available: 1 where both launches have kernels for d_head in the
 * calling thread's math mode, else 0; host only, launches nothing. */
CSN_API int csn_cross_attn_flash_available(int d_head);
CSN_API int csn_cross_attn_bwd_flash_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                                 const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                                 const float* lse, float* delta, float* dq, float* dk, float* dv, long long dq_eval_stride,
                                 long long dkv_eval_stride, int n_evals, int n_heads, int d_head, int n_queries, int n_keys,
                                 int score_pitch, float dropout_p, unsigned long long seed, void* stream);
CSN_API int csn_varlen_attn_bwd_flash_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                                  const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                                  const float* lse, float* delta, float* dq, float* dk, float* dv, long long dq_eval_stride,
                                  long long dkv_eval_stride, int n_evals, int n_heads, int d_head, int max_queries, int max_keys,
                                  const int* n_queries, const int* n_keys, int score_pitch, float dropout_p,
                                  unsigned long long seed, void* stream);

/* ---- (4) output projection + residual + LayerNorm, forward -------------------------------------------
 * z[c][n] = sum_D wfc[c][D] ctx[e][D][n] + xres[res_index[e]][c][n];  xhat = (z - mean_c z) * rstd,
 * rstd = 1/sqrt(var_c z + eps).   Replaces fc + residual + LayerNorm (csa_models.py:52,57,114-118) up to the
 * LayerNorm's affine (gamma, beta), which the caller applies (it is needed un-applied by the backward).
 *   xhat [n_evals][d_model][ld],  rstd [n_evals][n_points].
 * dropout_p / seed: train-mode dropout on the fc output before the residual add (csa_models.py:56,115);
 * mask = function of (seed, evaluation, channel, point, ld) — the backward entry regenerates it from the same values.
 * 0 = eval mode.
 * xhat_sum (optional) [n_evals][d_model]: sum over the points of every xhat row — n_points * the pooled descriptor
 * mean_n SSA(x) of csa_models.py:211-212, 218-219 before the affine.  With a workspace sum_ws of
 * n_evals * ceil(n_points / 256) * d_model floats (sum_ws_floats says how many there are) the 256-channel bf16x3 kernel forms
 * per-tile partial sums in its epilogue and a small kernel adds them in a fixed order; without one, or on the other kernels,
 * a streaming pass over xhat follows (dense maps only: xhat_eval_stride == d_model * ld).
 * csn_outproj_ln_workspace_floats: the sum_ws size with which the fused sums are taken on every kernel that has them (the
 * streaming kernel of the bf16x3 mode keeps one partial per work-group and evaluation it touches; a smaller workspace is
 * never an error — the streaming pass runs instead). */
CSN_API long long csn_outproj_ln_workspace_floats(int n_evals, int d_model, int d_inner, int n_points);
CSN_API int csn_outproj_ln_fwd_f32(const float* ctx, long long ctx_eval_stride, const float* wfc, const float* xres,
                           long long xres_shape_stride, const int* res_index, float* xhat,
                           long long xhat_eval_stride, float* rstd, int n_evals, int d_model, int d_inner, int ld,
                           int n_points, float eps, float dropout_p, unsigned long long seed, float* xhat_sum,
                           float* sum_ws, long long sum_ws_floats, void* stream);

/* ---- (5) output projection + LayerNorm, backward -------------------------------------------------------
 * dz   = dropout-mask * LayerNorm-backward(dxhat; xhat, rstd)   [n_evals][d_model][ld]  (d fc output)
 * dz_res = the same without the mask (d residual input); may be NULL when input gradients are not needed
 * dctx = wfc^T dz                                          [n_evals][d_inner][ld]
 * dwfc (+)= sum_{e,n} dz[e][:,n] ctx[e][:,n]^T             [d_model][d_inner]
 * wfc_t is wfc transposed, [d_inner][d_model] row-major.  `ws` is scratch of at least
 * csn_wgrad_workspace_floats(d_model, d_inner, n_evals, n_points) floats.  accumulate != 0 adds into dwfc.
 * The incoming gradient is  dxhat[e][c][n] (evaluations e < n_dense_evals only; the others have none)
 *                         + dxhat_rows[e][c] (optional, NULL = none): a term that is constant along the points — the
 * gradient of the pooled means (csa_models.py:212,219) — so that it never has to be expanded to a full map.
 * dxhat_scale (optional) [n_dense_evals][d_model] and dxhat_group (>= 1; 0 = 1): the dense term of evaluation e is
 *   dxhat_scale[e][c] * dxhat[e / dxhat_group][c][n]
 * — with dxhat = the gradient of the mixed features (dfeats of csn_mix_bwd_f32, one map per query shape), dxhat_group = the
 * evaluations mixed per shape and dxhat_scale = comp * gamma, the per-evaluation gradient maps of the mix (:233, :238) are
 * rebuilt on the fly and never travel through HBM. */
CSN_API int csn_outproj_ln_bwd_f32(const float* dxhat, const float* xhat, const float* rstd, long long eval_stride,
                           const float* ctx, long long ctx_eval_stride, const float* wfc_t, float* dz, float* dz_res,
                           float* dctx, float* dwfc, float* ws, long long ws_floats, int n_evals, int d_model,
                           int d_inner, int ld, int n_points, int accumulate, float dropout_p,
                           unsigned long long seed, int dctx_split, long long dctx_plane_stride,
                           const float* dxhat_rows, int n_dense_evals, const float* dxhat_scale, int dxhat_group,
                           void* stream);

/* ---- (5b) the same LayerNorm backward and dctx over a RANGE of evaluations, without the weight gradient ----
 * csn_outproj_lnb_f32 writes dz, dz_res (optional) and dctx of evaluations e_base .. e_base + n_evals - 1 of the maps — the
 * arguments and the arithmetic of (5), evaluation indices absolute (the dropout masks are keyed on them), dctx with the stride of
 * the maps.  A backward may so run in pieces, in any order, and finish with dwfc over all of dz through csn_project_wgrad_f32
 * (dout = dz, x = ctx: the contraction (5) ends with); every piece gives the bits of the one call.
 * It exists on the fused kernel only (math mode 1, fp32 maps, d_model = d_inner = 256): CSN_E_DIM elsewhere.
 * csn_outproj_lnb_workspace_floats(n_evals, ...) is 0 where a call over evaluations 0 .. n_evals - 1 would be refused, else the
 * floats of red_ws for the reductions below over that many evaluations.
 * rowdot / rowsum / red_ws (all three or none; then e_base = 0 and n_evals <= n_dense_evals a multiple of dxhat_group): the
 * reductions of csn_mix_bwd_f32 from the same pass over xhat and dxhat, on the raw dxhat (dfeats) values,
 *   rowdot[e][c] = sum_n dxhat[e / dxhat_group][c][n] xhat[e][c][n]      [n_evals][256]
 *   rowsum[g][c] = sum_n dxhat[g][c][n]                                  [n_evals / dxhat_group][256]
 * fp32 partial sums per work-group and evaluation in red_ws, added in fp64 in a fixed order (two calls give the same bits). */
CSN_API long long csn_outproj_lnb_workspace_floats(int n_evals, int d_model, int d_inner, int ld, int n_points);
CSN_API int csn_outproj_lnb_f32(const float* dxhat, const float* xhat, const float* rstd, long long eval_stride,
                        const float* wfc_t, float* dz, float* dz_res, float* dctx, int e_base, int n_evals, int d_model,
                        int d_inner, int ld, int n_points, float dropout_p, unsigned long long seed,
                        const float* dxhat_rows, int n_dense_evals, const float* dxhat_scale, int dxhat_group,
                        float* rowdot, float* rowsum, float* red_ws, long long red_ws_floats, void* stream);

/* ---- (6) projection weight gradient ----------------------------------------------------------------------
 * dw[r][c] (+)= scale * sum_{s,n} dout[s][r][n] * x[s][c][n]        (autograd of csa_models.py:103-105)
 * channels, n_points and both row pitches are multiples of 4 (CSN_E_ALIGN), rows is free; accumulate: scale applies to the new
 * term only. */
CSN_API int csn_project_wgrad_f32(const float* dout, long long dout_shape_stride, int ld_dout, const float* x,
                          long long x_shape_stride, int ld_x, float* dw, int rows, int channels, int n_shapes,
                          int n_points, float scale, int accumulate, float* ws, long long ws_floats,
                          void* stream);

/* Scratch floats needed by (5)/(6) for a [rows][cols] gradient reduced over n_maps maps of n_points points. */
CSN_API long long csn_wgrad_workspace_floats(int rows, int cols, int n_maps, int n_points);

/* ---- (7) retrieval measure for the shape kNN graph (csa_models.py:244-267) ------------------------------
 * r[i][j] = mean_n max_m cos(f1[i][n][:], f2[j][m][:]) over L2-normalised rows (eps 1e-12), for
 * POINT-MAJOR features f1 [s1][n1][channels], f2 [s2][n2][channels] as get_all_feats returns them
 * (csa_models.py:299).  ws: at least (s1*n1 + s2*n2) floats (inverse row norms) + s1*s2*n1 floats (per-point maxima): O(s1*s2),
 * so a caller with many shapes scores the query shapes in row chunks (csn_amd.functional.retrieval_measure does).  Any pair
 * count is accepted up to ceil(n1/128)*s1*s2 < 2^31 work-groups (CSN_E_ARG beyond). */
CSN_API int csn_retrieval_measure_f32(const float* f1, const float* f2, float* out, int s1, int n1, int s2, int n2,
                              int channels, float* ws, long long ws_floats, void* stream);

/* ---- (8) pooled descriptors and the cross-shape mix (csa_models.py:211-212, 218-219, 232-240) --------------
 * csn_rowsum_f32 : out[r] = sum_{n < n_points} x[r*ld + n]   (fp64 accumulation; the caller divides by n_points to
 *                  get the mean-over-points SSA descriptor of :212 / :219).
 * csn_mix_fwd_f32: feats[b][c][n] = gamma[c] * sum_k comp[b][k] * xhat[b*k1 + k][c][n] + beta[c] * sum_k comp[b][k]
 *                  i.e. sum_k comp_k * LayerNorm-affine(xhat_k): the compatibility-weighted sum of :233 and :238.
 * csn_mix_bwd_f32: dxhat[b*k1 + k][c][n] = comp[b][k] gamma[c] dfeats[b][c][n];
 *                  rowdot[b][k][c] = sum_n dfeats[b][c][n] xhat[b*k1+k][c][n];  rowsum[b][c] = sum_n dfeats[b][c][n]
 *                  (fp64 accumulation) from which d comp, d gamma, d beta follow with O(B*k1*C) host-side math.
 *                  dxhat (and dxhat_self) NULL: the reductions only — the maps are then rebuilt inside
 *                  csn_outproj_ln_bwd_f32 (dxhat_scale / dxhat_group).
 * xhat_self / dxhat_self != NULL: the k = 0 maps (the shape's own evaluation) live in their own tensors [b][c][n] and
 * xhat / dxhat hold the k1 - 1 others, [b*(k1-1) + k-1] — the form the overlapped multi-GPU path produces (own shapes are
 * evaluated while the neighbour exchange is in flight), so that no concatenation of the two is ever built.
 * All maps dense channel-major [..][channels][n_points], n_points % 4 == 0, k1 <= 8. */
CSN_API int csn_rowsum_f32(const float* x, float* out, long long rows, int n_points, long long ld, void* stream);
CSN_API int csn_mix_fwd_f32(const float* xhat, const float* comp, const float* gamma, const float* beta, float* feats,
                    int n_shapes, int k1, int channels, int n_points, const float* xhat_self, void* stream);
CSN_API int csn_mix_bwd_f32(const float* dfeats, const float* xhat, const float* comp, const float* gamma, float* dxhat,
                    float* rowdot, float* rowsum, int n_shapes, int k1, int channels, int n_points, const float* xhat_self,
                    float* dxhat_self, void* stream);

/* ---- (9) the compatibility head (csa_models.py:222-230) -----------------------------------------------------
 * comp[b][k] = softmax_k < normalize(wq y[b][0] + bq), normalize(wk key(b, k) + bk) >  over the k1 = K+1 pooled descriptors
 * y (n_shapes, k1, channels) of every query shape (the shape itself in slot 0), F.normalize's eps = 1e-12, channels <= 256,
 * k1 <= 8.  reference_layout != 0: the key rows are taken the way the reference's bookkeeping takes them for B > 1 — the key
 * descriptors stacked neighbour-major and re-viewed as (B, k1, C) (csa_models.py:213,220,227): key(b, k) = y[(b k1 + k) % B]
 * [(b k1 + k) / B]; 0: key(b, k) = y[b][k].
 * Every sum accumulates in fp64 (the head's gradients are differences of nearly equal descriptors; 63 MFLOP).
 * Forward: wq_t / wk_t are the nn.Linear weights TRANSPOSED ([in][out]); save_u (n_shapes, k1 + 1, channels) and save_norm
 * (n_shapes, k1 + 1) keep the normalised vectors and the norms for the backward, as DOUBLES.
 * Backward: wq / wk as stored ([out][in]); ws >= 2 n_shapes (k1 + 1) channels DOUBLES of scratch; writes the gradients
 * dpooled (n_shapes, k1, channels), dwq / dwk (channels, channels) and dbq / dbk (channels) — overwritten, not accumulated;
 * sums over the shapes run in a fixed order (bitwise reproducible). */
CSN_API int csn_compat_fwd_f32(const float* pooled, const float* wq_t, const float* bq, const float* wk_t, const float* bk, float* comp,
                       double* save_u, double* save_norm, int n_shapes, int k1, int channels, int reference_layout, void* stream);
CSN_API int csn_compat_bwd_f32(const float* dcomp, const float* comp, const double* save_u, const double* save_norm, const float* pooled,
                       const float* wq, const float* wk, double* ws, long long ws_doubles, float* dpooled, float* dwq, float* dbq,
                       float* dwk, float* dbk, int n_shapes, int k1, int channels, int reference_layout, void* stream);

/* ---- (10) the loss the layers are trained with (csa_training.py:94-108) -----------------------------------------------
 * The reference transposes the logits to [point][class], gathers the points with label > mask and calls F.cross_entropy and
 * an argmax accuracy on the selection.  Here the class-major logits [shape][class][ld] (the layout the logit layer writes,
 * csa_models.py:151) are read where they lie:
 *   forward   stats[0] = mean over the counted points (mask < label < n_classes) of lse - z[label], stats[1] = the fraction of
 *             them whose first arg-max class is the label, stats[2] = their number (0 counted points: 0 / 0 = nan, as the
 *             reference's empty selection gives); lse [n_shapes][n_points] is kept for the backward.  ws: scratch of
 *             csn_masked_ce_workspace_bytes(n_shapes, n_points) bytes, 8-byte aligned (per-block fp64 partial sums, added in a
 *             fixed order: bitwise reproducible).
 *   backward  dlogits[s][c][n] = counted ? (exp(z - lse) - [c == label]) * grad_out[0] / stats[2] : 0, every class row of
 *             every shape written; any point count, pitch and alignment (16-byte accesses where n_points, ld, dld and the shape
 *             strides are % 4 == 0 and logits, lse, dlogits 16-byte aligned; one point per thread otherwise).  A logit of -inf
 *             is a probability of zero (also as a point's first class).
 *   metrics   csn_masked_ce_metrics_fwd_f32: the forward pass, keeping what it forms on the way (the validation and test
 *             mode's loss, predictions and Part-IoU counts from one read of the logits).  stats and lse (may be NULL here)
 *             are bit for bit the forward's; pred (int32 [n_shapes][n_points], may be NULL) = every point's first arg-max
 *             class, masked or not; counts (int32 [n_shapes][n_classes][3], overwritten) = per shape and class the
 *             intersection / ground-truth / prediction counts over the points with label > mask (IoU_per_shape's selection,
 *             csa_training.py:110-134, without the loss's upper bound): such a point adds 1 to pr[pred], with label <
 *             n_classes also 1 to gt[label], and with pred == label also 1 to inter[label]; union = gt + pr - inter.
 *             Integer atomics only: exact and reproducible.  ws as for the forward
 *             (csn_masked_ce_metrics_workspace_bytes); csn_masked_ce_bwd_f32 takes its lse and stats.
 * labels are int64 (torch.long), label_shape_stride elements apart per shape. */
CSN_API long long csn_masked_ce_workspace_bytes(int n_shapes, int n_points);
CSN_API int csn_masked_ce_fwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels, long long label_shape_stride,
                          int n_shapes, int n_classes, int n_points, int mask, float* lse, void* ws, long long ws_bytes,
                          float* stats, void* stream);
CSN_API int csn_masked_ce_bwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels, long long label_shape_stride,
                          int n_shapes, int n_classes, int n_points, int mask, const float* lse, const float* stats,
                          const float* grad_out, float* dlogits, long long dshape_stride, int dld, void* stream);
CSN_API long long csn_masked_ce_metrics_workspace_bytes(int n_shapes, int n_classes, int n_points);
CSN_API int csn_masked_ce_metrics_fwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels,
                          long long label_shape_stride, int n_shapes, int n_classes, int n_points, int mask,
                          float* lse /* may be NULL */, int* pred /* may be NULL */, int* counts,
                          void* ws, long long ws_bytes, float* stats, void* stream);

/* ---- (11) the MinkowskiNet cross-shape head on ragged shape batches (MinkowskiNet/models/hrnet.py:359-423, 472-490) -------
 * A MinkowskiNet batch packs the points of its shapes row after row; shape b owns the rows offsets[b] .. offsets[b+1] - 1
 * (the cu_seqlens of rows sorted by shape, every shape >= 1 point).  Every offsets / counts array is passed TWICE, with the
 * same numbers: *_host (host memory: validated and used to size the grid before anything is enqueued) and the device copy
 * the kernels read.  Maps xhat / dxhat are the varlen attention's channel-major, pre-affine LayerNorm outputs
 * [n_evals][channels][ld] at eval_stride floats per evaluation (ld, eval_stride % 4, 16-byte aligned); evaluation e has
 * counts[e] real points — the points [counts[e], ld) enter no sum and are written as zero in every gradient map (the varlen
 * attention runs round-up-4(counts[e]) queries: the points up to that bound hold real, non-zero values).  The points
 * [counts[e], ld) of xhat must still be FINITE: csn_ragged_mix_bwd_f32 forms 0 * xhat for the points between a shape's count
 * and the end of its last 64-point tile, so an inf or nan there reaches rowdot (the varlen attention leaves finite values).
 * Evaluation order of the mix: ev(b, 0) = b (SSA of query shape b), ev(b, j >= 1) = cross_first + (j-1) n_shapes + b
 * (MHA(q_b, k_{j,b}, k_{j,b})); k1 = K + 1 <= 8.  All sums accumulate in fp64 in a fixed order (bitwise reproducible).
 * csn_ragged_pool_f32      pooled[e][c] = gamma[c] mean_{n < counts[e]} xhat[e][c][n] + beta[c]  (hrnet.py:380-381, 388-389:
 *                          torch.mean of the affine SSA rows); mean (optional) [e][c] = the mean before the affine.
 * csn_ragged_pool_bwd_f32  dxhat[e][c][n] = (accumulate ? dxhat[e][c][n] : 0) + (n < counts[e] ? gamma[c] dpooled[e][c] / counts[e]
 *                          : 0) for n < ld.
 * csn_ragged_mix_fwd_f32   out[offsets[b] + n][c] = sum_j comp[b][j] (gamma[c] xhat[ev(b,j)][c][n] + beta[c]), n < the shape's
 *                          points, POINT-MAJOR at ld_out floats per row (hrnet.py:397-411; with out = the second half of the output
 *                          layer's (rows, 2 channels) input the concatenation of :423 costs nothing).  k1 = 1, comp = 1: the SSA
 *                          rows themselves (:366-368, K = 0).  Needs the longest shape <= ld.
 * csn_ragged_mix_bwd_f32   dxhat[ev(b,j)][c][n] = comp[b][j] gamma[c] dout[offsets[b] + n][c] (0 from the shape's points to ld);
 *                          rowdot[b][j][c] = sum_n dout[..][c] xhat[ev(b,j)][c][n], rowsum[b][c] = sum_n dout[..][c] (DOUBLES),
 *                          from which d comp, d gamma and d beta follow with O(n_shapes k1 channels) math.
 *                          ws >= n_shapes (k1 + 1) ceil(ld / 64) channels doubles (per-64-point-tile partial sums).
 * csn_ragged_retrieval_f32 out[i][j] = mean_{n < n1_i} max_{m < n2_j} cos(f1[offsets1[i] + n], f2[offsets2[j] + m])  (hrnet.py:472-490
 *                          for every (query, key) pair at once; point-major rows, channels % 4, the fp32 matrix-core arithmetic of
 *                          (7); the rows are normalised with max(|x|, 1e-12), where the reference divides by the raw norm: they
 *                          differ only for an all-zero row).  No n x m matrix and no padding: a work-group of 128 query points
 *                          exits at once past its shape, the candidate sweep stops at the candidate's points.
 *                          ws >= N1 + N2 + s1 s2 ceil(max n1_i / 128) floats (inverse row norms + per-tile partial sums). */
CSN_API int csn_ragged_pool_f32(const float* xhat, long long eval_stride, int ld, const int* counts_host, const int* counts,
                        int n_evals, int channels, const float* gamma, const float* beta, float* pooled, float* mean, void* stream);
CSN_API int csn_ragged_pool_bwd_f32(const float* dpooled, const float* gamma, const int* counts_host, const int* counts, int n_evals,
                            int channels, float* dxhat, long long eval_stride, int ld, int accumulate, void* stream);
CSN_API int csn_ragged_mix_fwd_f32(const float* xhat, long long eval_stride, int ld, int n_evals, int cross_first,
                           const int* offsets_host, const int* offsets, int n_shapes, int k1, int channels, const float* comp,
                           const float* gamma, const float* beta, float* out, long long ld_out, void* stream);
CSN_API int csn_ragged_mix_bwd_f32(const float* dout, long long ld_dout, const float* xhat, long long eval_stride, int ld, int n_evals,
                           int cross_first, const int* offsets_host, const int* offsets, int n_shapes, int k1, int channels,
                           const float* comp, const float* gamma, float* dxhat, double* rowdot, double* rowsum, double* ws,
                           long long ws_doubles, void* stream);
CSN_API int csn_ragged_retrieval_f32(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                             const int* offsets2_host, const int* offsets2, int s2, int channels, float* out, float* ws,
                             long long ws_floats, void* stream);

/* ---- (11b) fp16 screen and pair-list form of the ragged retrieval measure: top-K retrieval without every pair in fp32 ----
 * Offsets as in (11).  Independent of the math mode.
 * csn_ragged_retrieval_screen_f16  the arguments and the meaning of csn_ragged_retrieval_f32, out[i][j] within
 *                          csn_retrieval_screen_eps(channels) of what that entry writes: every row normalised in fp32 (the
 *                          same max(|x|, 1e-12) clamp, behind an exact power-of-two scaling by the row's largest element),
 *                          times 2^7, rounded ONCE to fp16 (channels zero-padded to a multiple of 32), one
 *                          v_mfma_f32_32x32x16_f16 per product, fp32 accumulation, the product scaled back by 2^-14 (exact).
 *                          A work-group keeps its 128 query points in LDS and streams the candidate's points through a
 *                          double-buffered image; partial sums per (pair, tile) are added in tile order in fp64: no atomics,
 *                          two calls give the same bits.  channels % 4 == 0 and round-up-32(channels) <= 288 (CSN_E_DIM
 *                          beyond: the three images no longer fit one CU's LDS).  ws >=
 *                          csn_retrieval_screen_workspace_floats(N1, N2, s1, s2, max n1_i, channels) floats, 16-byte aligned.
 * csn_retrieval_screen_eps  the bound: |screen - fp32 measure| <= eps for every pair whose rows the fp32 measure can normalise
 *                          (a sum of squares inside the fp32 range; a caller keeps other rows out of the screen's decisions).
 *                          DERIVED (DESIGN.md "fp16 screen of the shape graph"), a function of the channel count alone:
 *                          about 2^-10 + (7 channels + 350) 2^-24 (1.10e-3 at 256 channels).  It holds whether the matrix
 *                          unit flushes fp16 subnormal operands or not: after the 2^7 scaling an element in that range
 *                          moves a cosine by < 2^-21.
 * csn_ragged_retrieval_pairs_f32  out[p] = the fp32 measure of the pair (pairs[2p], pairs[2p+1]) for n_pairs listed pairs
 *                          (DEVICE int32, any order, repeats allowed): the work-groups of csn_ragged_retrieval_f32 with the
 *                          pair looked up — the same sums in the same order, the same bits.  An index outside
 *                          [0, s1) x [0, s2) reads nothing and writes nan.
 *                          ws >= N1 + N2 + n_pairs ceil(max n1_i / 128) floats. */
CSN_API long long csn_retrieval_screen_workspace_floats(long long n1_rows, long long n2_rows, int s1, int s2, int max_n1, int channels);
CSN_API float csn_retrieval_screen_eps(int channels);
CSN_API int csn_ragged_retrieval_screen_f16(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                                    const int* offsets2_host, const int* offsets2, int s2, int channels, float* out, float* ws,
                                    long long ws_floats, void* stream);
CSN_API int csn_ragged_retrieval_pairs_f32(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                                   const int* offsets2_host, const int* offsets2, int s2, int channels, const int* pairs,
                                   long long n_pairs, float* out, float* ws, long long ws_floats, void* stream);

/* ---- (12) loss, predictions and IoU counts of the MinkowskiNet head (MinkowskiNet/lib/trainer_csn.py:188-224, 400-500;
 *           lib/utils.py:64-176) -----------------------------------------------------------------------------------------------
 * The reference's loop computes nn.CrossEntropyLoss(ignore_index) (trainer_csn.py:406, 471), the prediction
 * torch.max(output[:, 1:], 1)[1] + 1 (:221, :466), precision_at_one_partnet (utils.py:64-75) and calculate_iou (utils.py:78-110)
 * one after the other, the last two on the host.  Here ONE pass reads the logits where the head leaves them: POINT-MAJOR ragged
 * rows logits[n_rows][ld] (fp32, n_classes <= ld, any ld and alignment: 16-byte accesses where ld <= 59 and the base is 16-byte
 * aligned), labels[n_rows] int64, and segments offsets[n_segments + 1] passed twice as in (11) (every segment >= 1 row, from 0 to
 * n_rows: the shapes of the batch for the per-shape metric, {0, n_rows} for the reference's grouping of a whole test batch as
 * one "model", trainer_csn.py:474).  n_classes >= 2; ignore_label is any int (the reference's default is 255).
 *   A row is COUNTED when label != ignore_label and 0 <= label < n_classes; BAD when its label is neither the ignore label nor
 *   in [0, n_classes) (torch raises for these; here they enter nothing but stats[3], so a caller can raise without a
 *   synchronisation per step); otherwise IGNORED.
 * csn_ragged_seg_fwd_f32 writes
 *   lse[n]      log sum_{c < n_classes} exp(z[n][c])                                    (every row)
 *   nll[n]      the row's loss lse - z[label] of a counted row, 0 otherwise.  It is formed as log1p(sum of the exponentials
 *               without the maximum's) + (max - z[label]): two non-negative terms, where lse - z[label] cancels for a confident
 *               row (a loss of 1e-3 is below one part in 1e4 of an lse of 4).  The loss sums these; the backward reads them.
 *   pred[n]     1 + argmax_{1 <= c < n_classes} z[n][c], the FIRST maximum on ties      (every row, int32)
 *   stats[0]    mean over the counted rows of lse - z[label]  (none: 0 / 0 = nan, as torch gives)
 *   stats[1..3] the number of counted rows, of counted rows with pred == label or label == 0 (utils.py:69-70), of bad rows
 *               (DOUBLES, 8-byte aligned)
 *   counts[s][i][0..2]  (int32, overwritten) with p' = (label == 0 ? 0 : pred) over the rows of segment s that are not bad:
 *               inter = #(label == i and p' == i), gt = #(label == i), pr = #(p' == i); union = gt + pr - inter.  An IGNORED
 *               row keeps its prediction and enters pr (hence the union), as calculate_iou has it: only ground == 0 is zeroed.
 *   ws: csn_ragged_seg_workspace_bytes(n_rows) bytes, 8-byte aligned (per-work-group fp64 partial sums, added in a fixed order:
 *   the loss is bitwise reproducible; the counts are integer atomics: exact in any order).
 * csn_ragged_seg_bwd_f32  dlogits[n][c] = counted ? (exp(z[n][c] - lse[n]) - [c == label]) * grad_out[0] / stats[1] : 0 for
 *   c < n_classes, rows dld floats apart (n_classes <= dld); the columns [n_classes, dld) are LEFT UNTOUCHED.  A logit of -inf is
 *   a probability of zero, as in (10).  The label's own entry is expm1(-nll[n]) (exp(z - lse) - 1 cancels).  16-byte accesses where ld == dld == n_classes and both bases are 16-byte aligned. */
CSN_API long long csn_ragged_seg_workspace_bytes(int n_rows);
CSN_API int csn_ragged_seg_fwd_f32(const float* logits, int n_rows, int ld, const long long* labels, const int* offsets_host,
                           const int* offsets, int n_segments, int n_classes, int ignore_label, float* lse, float* nll, int* pred,
                           double* stats, int* counts, void* ws, long long ws_bytes, void* stream);
CSN_API int csn_ragged_seg_bwd_f32(const float* logits, int n_rows, int ld, const long long* labels, int n_classes, int ignore_label,
                           const float* lse, const float* nll, const double* stats, const float* grad_out, float* dlogits, int dld,
                           void* stream);

/* ---- (13) fc_layer of the MinkowskiNet head: 1x1 convolution + BatchNorm + ReLU (MinkowskiNet/models/hrnet.py:332-339, applied
 *           to the query batch at :439 and to every key batch at :451) -----------------------------------------------------------
 * The reference's fc_layer is MinkowskiConvolution(kernel_size = 1, bias) + MinkowskiBatchNorm + MinkowskiReLU on the concatenated
 * backbone map (416 / 480 / 992 channels) down to d_model.  On the dense feature rows this is nn.Linear + nn.BatchNorm1d + ReLU;
 * ONE CALL IS ONE BatchNorm BATCH (the reference calls the layer once per batch).  Everything is POINT-MAJOR fp32:
 *   x[n_rows][ld_x]  (c_in <= ld_x),  w[c_out][c_in] row-major (contiguous),  bias[c_out] (may be NULL),  gamma / beta /
 *   running_mean / running_var / mean / invstd [c_out],  y[n_rows][ld_y],  z[n_rows][ld_z],  dy[n_rows][ld_dy],  dx[n_rows][ld_dx],
 *   dw[c_out][c_in] (contiguous),  dbias / dgamma / dbeta [c_out].  Columns of a row beyond its width are neither read as data nor
 *   written.
 * Geometry: n_rows >= 1 (no % 4 requirement); c_in % 32 == 0, 32 <= c_in <= 1024; c_out in {32, 64, 96, 128, 256} (CSN_E_DIM);
 * every pitch % 4 == 0 (CSN_E_ALIGN), >= its width (CSN_E_ARG) and <= 2^20 (CSN_E_DIM); x, w, y, z, dy, dx, dw, ws 16-byte aligned
 * (CSN_E_PTR).  training != 0 with n_rows == 1 returns CSN_E_ARG (no variance; torch refuses it too).  All of this is checked on the
 * host before any launch.  ws: csn_rows_fc_workspace_bytes(n_rows, c_in, c_out, training, backward) bytes (backward = 0 for the
 * forward call, 1 for the backward call; 0 for an eval forward, which takes ws = NULL).
 * csn_rows_fc_fwd_f32, training != 0:
 *   z = x w^T + bias;  mean, var (biased) per column over the n_rows rows;  invstd = 1 / sqrt(var + eps);
 *   y = max(0, gamma (z - mean) invstd + beta);  running_mean <- (1 - momentum) running_mean + momentum mean;
 *   running_var <- (1 - momentum) running_var + momentum var n / (n - 1)   (either running pointer may be NULL: not tracked).
 *   z, mean and invstd are written for the backward.  The column statistics are (mean, M2) pairs of 32-row tiles formed in the
 *   product's epilogue and merged by Chan's formula in fp64 in a fixed order.
 * csn_rows_fc_fwd_f32, training == 0: ONE launch; the product's epilogue applies s = gamma / sqrt(running_var + eps),
 *   t = beta + (bias - running_mean) s and the ReLU: only y is written (z, mean, invstd, ws may be NULL).
 * csn_rows_fc_bwd_f32: with g' = dy [y > 0] (y is the forward's output: the mask is the forward's own) and xhat = (z - mean) invstd,
 *   dgamma = sum_n g' xhat,  dbeta = sum_n g'                                             (always written)
 *   training: dz = gamma invstd (g' - mean_n g' - xhat mean_n (g' xhat));  stat_mean / stat_scale = the forward's mean / invstd
 *   eval:     dz = g' gamma / sqrt(running_var + eps);  stat_mean / stat_scale = running_mean / running_var; z is not read (NULL):
 *             the product x w^T + bias is formed again into ws
 *   dx = dz w,  dw = dz^T x (split-K over the rows, slabs added in order),  dbias = sum_n dz — each skipped when its pointer is NULL.
 *   Column sums are fp64 partials of 64-row chunks added in a fixed order.
 * No floating-point atomics: two identical calls give the same bits.  Math mode 0 runs the three products on the exact fp32 matrix
 * instruction, mode 1 as bf16x3; modes 2 / 3 run as mode 1, like (3b), unless csn_set_thread_rows16(1) selects their single-product
 * instances (mode 3: the forward only; csn_rows_fc_bwd_f32 then returns CSN_E_ARG). */
CSN_API long long csn_rows_fc_workspace_bytes(int n_rows, int c_in, int c_out, int training, int backward);
CSN_API int csn_rows_fc_fwd_f32(const float* x, long long ld_x, int n_rows, int c_in, int c_out, const float* w, const float* bias,
                        const float* gamma, const float* beta, float* running_mean, float* running_var, float eps, float momentum,
                        int training, float* y, long long ld_y, float* z, long long ld_z, float* mean, float* invstd, void* ws,
                        long long ws_bytes, void* stream);
CSN_API int csn_rows_fc_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const float* z, long long ld_z,
                        const float* x, long long ld_x, int n_rows, int c_in, int c_out, const float* w, const float* bias,
                        const float* gamma, const float* stat_mean, const float* stat_scale, float eps, int training, float* dx,
                        long long ld_dx, float* dw, float* dbias, float* dgamma, float* dbeta, void* ws, long long ws_bytes,
                        void* stream);

/* ---- (14) sparse 3D convolution on voxel rows (MinkowskiNet/models/hrnet.py:39-53 the stem, :89-111 the stride-2 and transposed
 *           convolutions between branches, :233-239 the blocks; models/modules/resnet_block.py:22-57) ----------------------------
 * Every convolution of the HRNet backbone is MinkowskiConvolution / MinkowskiConvolutionTranspose on voxel coordinates: kernel 3 or
 * 5 at stride 1, kernel 3 at stride 2, and the transposed kernel 3 at stride 2.  All of them are ONE gather-GEMM over a KERNEL MAP
 * the caller builds (csn_amd.minkowski_conv.build_kernel_map):
 *   table[kv][n_out] int32 — table[k][j] is the input row that feeds output row j at kernel offset k, or -1 (no voxel there).
 *   y[j] = sum_k x[table[k][j]] W[k] + bias
 * Everything is POINT-MAJOR fp32: x[n_in][ld_x] (c_in <= ld_x), w[kv][c_in][c_out] (contiguous; MinkowskiEngine's `kernel`),
 * bias[c_out] (may be NULL), y[n_out][ld_y], dy[n_out][ld_dy], dx[n_in][ld_dx], dw[kv][c_in][c_out] (contiguous), dbias[c_out].
 * Columns of a row beyond its width are neither read as data nor written.  Any negative table entry reads as "no voxel".  An
 * entry >= n_in is the caller's error: the buffer range check keeps it from being dereferenced outside x, its contribution is undefined.
 * Geometry: n_in, n_out >= 1 (no % 4 requirement; CSN_E_ARG); kv in {1, 27, 125}, c_in % 32 == 0 and c_out % 32 == 0, both in
 * [32, 256] (CSN_E_DIM); every pitch % 4 == 0 (CSN_E_ALIGN), >= its width (CSN_E_ARG), <= 2^20 and rows * pitch * 4 < 2 GiB, the
 * buffer window of the gathers (CSN_E_DIM); x, w, y, dy, dx, dw, ws 16-byte aligned, the tables 4-byte (CSN_E_PTR).  All of this is
 * checked on the host before any launch.  ws (backward only): csn_sparse_conv_workspace_bytes(..., backward = 1) bytes
 * (CSN_E_WORKSPACE); the forward takes none (backward = 0 returns 0).
 * csn_sparse_conv_fwd_f32: one launch.  Reads x, table, w, bias; writes y (every row by exactly one wave); nothing else.  An offset
 *   at which no row of a work-group's 128-row tile has a neighbour is skipped whole by that work-group.
 * csn_sparse_conv_bwd_f32: with fwd_table[kv][n_out] as above and bwd_table[kv][n_in] — bwd_table[k][i] is the output row that
 *   input row i feeds at offset k, or -1; bwd_table NULL with n_in == n_out means the stride-1 identity bwd[k] = fwd[kv - 1 - k]:
 *   the kernel walks fwd_table in reversed offset order and no second table exists (n_in != n_out: CSN_E_ARG) —
 *   dx = sum_k dy[bwd_table[k][i]] W[k]^T    the forward kernel on (dy, bwd_table, W^T); reads dy, bwd_table, w
 *   dw[k] = sum_j x[fwd_table[k][j]]^T dy[j]  split-K over chunks of output rows, slabs added in chunk order; reads x, fwd_table, dy
 *   dbias = sum_j dy[j]                       fp64 partials of 64-row chunks added in chunk order; reads dy
 *   — each skipped when its pointer is NULL (its own inputs may then be NULL too), the others are unchanged by that.
 * No floating-point atomics: two identical calls give the same bits.  Math mode 0 runs the products on the exact fp32 matrix
 * instruction, mode 1 as bf16x3; modes 2 / 3 run as mode 1, like (13), unless csn_set_thread_rows16(1) selects their single-product
 * instances (mode 3: the forward only; csn_sparse_conv_bwd_f32 then returns CSN_E_ARG). */
CSN_API long long csn_sparse_conv_workspace_bytes(int n_in, int n_out, int kv, int c_in, int c_out, int backward);
CSN_API int csn_sparse_conv_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in, int c_out,
                            const float* w, const float* bias, float* y, long long ld_y, void* stream);
CSN_API int csn_sparse_conv_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_in, int n_out, int kv, int c_in,
                            int c_out, const int* fwd_table, const int* bwd_table, const float* w, float* dx, long long ld_dx,
                            float* dw, float* dbias, void* ws, long long ws_bytes, void* stream);

/* ---- (15) the HRNet backbone's fused tail: convolution with a BatchNorm statistics epilogue, and normalise + sum + add + activate
 *           (MinkowskiNet/models/hrnet.py:124-131 the stem, :157-161 the branch sums, :308-326 the final transitions;
 *           models/modules/resnet_block.py:40-57 the block) --------------------------------------------------------------------
 * Every normalised convolution of the backbone (47 in HRNetSimCSN3S) is followed by a ReLU, a residual add or a sum over branches.
 * Two entry points cover all of it.  Everything is POINT-MAJOR fp32 with pitches as in (14): widths % 32 == 0 in [32, 256]
 * (CSN_E_DIM); every pitch % 4 == 0 (CSN_E_ALIGN), >= the width (CSN_E_ARG), <= 2^20 and rows * pitch * 4 < 2 GiB (CSN_E_DIM); maps
 * and ws 16-byte aligned (CSN_E_PTR); per-column vectors [channels] fp32.  All of this is checked on the host before any launch.
 * No floating-point atomics: every reduction has a fixed order, two identical calls give the same bits.
 *
 * (15a) csn_sparse_conv_stats_fwd_f32: z = gather-GEMM(x, table, w) exactly as csn_sparse_conv_fwd_f32 with bias = NULL — the SAME
 *   bits in the same math mode; the epilogue only adds — plus the BatchNorm statistics of z over its n_out rows:
 *   mean[c], invstd[c] = 1 / sqrt(var_biased + eps);  running_mean <- (1 - momentum) running_mean + momentum mean;
 *   running_var <- (1 - momentum) running_var + momentum var n / (n - 1)   (either running pointer may be NULL: not tracked).
 *   The product's epilogue forms (mean, M2) of each wave's <= 32 rows from the accumulators in two passes over the registers; the
 *   partials are merged by Chan's formula in fp64 in a fixed order, as in (13).  n_out == 1: CSN_E_ARG (no variance).
 *   ws: csn_sparse_conv_stats_workspace_bytes(n_out, c_out) bytes (CSN_E_WORKSPACE).  Math modes as in (14).
 *   Its backward is csn_sparse_conv_bwd_f32 (the statistics are taken up by (15b)'s dz).
 *
 * (15b) csn_rows_bn_act_fwd_f32:  y = act( sum_{m < n_terms} (gamma_m (z_m - mean_m) s_m + beta_m) + r ),  n_terms in {1, 2, 3}
 *   (CSN_E_ARG otherwise), r an optional residual map (NULL: none), act = ReLU (relu != 0) or the identity.  The terms cross the
 *   ABI as ONE host struct of arrays, CsnBnTerms: entry m of every array belongs to term m, entries >= n_terms are ignored.
 *   training != 0: s_m = scale[m] is the invstd of (15a), mean[m] its mean.  training == 0: mean[m] / scale[m] are the running mean
 *   / variance and s_m = 1 / sqrt(scale[m] + eps), as in (13).  Forward reads z, ld_z, mean, scale, gamma, beta of each term.
 *   y may be a column block of a wider buffer (ld_y > channels): columns outside [0, channels) of a row are not written.
 * csn_rows_bn_act_bwd_f32: g' = dy [y > 0] with the forward's own y (relu == 0: g' = dy, y may be NULL);
 *   dr = g';  per term dgamma[m] = sum_n g' xhat_m,  dbeta[m] = sum_n g',  xhat_m = (z_m - mean_m) s_m;
 *   training: dz[m] = gamma_m s_m (g' - mean_n g' - xhat_m mean_n(g' xhat_m))  — the complete BatchNorm gradient;
 *   eval:     dz[m] = g' gamma_m s_m.
 *   Any output whose pointer is NULL (dr, dz[m], dgamma[m], dbeta[m]) is skipped; beta is not read.  Pass 1 reads dy and y ONCE for
 *   all terms; column sums are fp64 partials of 64-row chunks added in a fixed order.
 *   ws: csn_rows_bn_act_workspace_bytes(n_rows, channels, n_terms) bytes (backward only; the forward takes none). */
typedef struct CsnBnTerms {
  const float* z[3];      long long ld_z[3];   /* the maps [n_rows][ld_z] */
  const float* mean[3];   const float* scale[3];
  const float* gamma[3];  const float* beta[3];
  float* dz[3];           long long ld_dz[3];  /* backward outputs, each may be NULL */
  float* dgamma[3];       float* dbeta[3];
} CsnBnTerms;
CSN_API long long csn_sparse_conv_stats_workspace_bytes(int n_out, int c_out);
CSN_API int csn_sparse_conv_stats_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                  int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                  float* running_mean, float* running_var, float eps, float momentum, void* ws, long long ws_bytes,
                                  void* stream);
CSN_API long long csn_rows_bn_act_workspace_bytes(int n_rows, int channels, int n_terms);
CSN_API int csn_rows_bn_act_fwd_f32(const CsnBnTerms* terms, int n_terms, int n_rows, int channels, int training, float eps,
                            const float* r, long long ld_r, int relu, float* y, long long ld_y, void* stream);
CSN_API int csn_rows_bn_act_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const CsnBnTerms* terms,
                            int n_terms, int n_rows, int channels, int training, float eps, int relu, float* dr, long long ld_dr,
                            void* ws, long long ws_bytes, void* stream);

/* ---- (16) point fields: voxelised features, interpolation of a voxel map onto points and its adjoint (MinkowskiNet/lib/
 *           trainer_csn.py:236-260 ME.TensorField(...).sparse(), :200-205 and :463-471 soutput.interpolate(field)) ----------------
 * The reference's loss and metrics live on POINTS: a batch's points are quantised to voxels, the network runs on the voxel rows
 * and its logits are interpolated back.  csn_amd.minkowski_field.PointField builds the index arrays (plumbing); the three entry
 * points below are the arithmetic.  Everything is POINT-MAJOR fp32 in every math mode (there is no matrix product here):
 *   coords[n_points][4] = [b, x, y, z] in voxel units (contiguous, 16-byte aligned: CSN_E_PTR);
 *   home[n_points] int32: the voxel row of [b, floor(x), floor(y), floor(z)];
 *   vox_ptr[n_voxels + 1], vox_pts[n_points] int32: the points of every voxel as a CSR, ascending inside a voxel;
 *   table[27][n_voxels] int32: the kernel-3 stride-1 map of (14) on the voxel set (-1: no voxel) — the row of v + c is
 *   table[13 + cx + 3 cy + 9 cz][v], the row of v - c is table[13 - cx - 3 cy - 9 cz][v], c in {0, 1}^3;
 *   z[n_voxels][ld_z], y[n_points][ld_y], dy[n_points][ld_dy], dz[n_voxels][ld_dz], feats[n_points][ld_feats], out[n_voxels][ld_out].
 * Any pitch >= its width; columns of a row beyond the width are neither read nor written.  16-byte accesses where both maps of a
 * call are 16-byte aligned and both pitches % 4 == 0 (a width % 4 != 0 then ends in a scalar tail), one element per access
 * otherwise.  Host-side checks before any launch: a NULL pointer, n_points < 1, n_voxels < 1 or a pitch below its width:
 * CSN_E_ARG; channels outside [1, 1024] ([1, 64] for the mean): CSN_E_DIM; a map or index array off 4 bytes: CSN_E_PTR.
 * An index outside its array is never dereferenced: it reads as "no voxel" / is skipped (its contribution is the caller's error).
 * (16a) csn_voxel_mean_f32: out[v] = (sum_{p in voxel v, ascending} feats[p]) / count   (n_voxels <= n_points).
 * (16b) csn_point_interp_fwd_f32: t = xyz - floor(xyz) (the fp32 difference) and
 *   y[p] = sum_{c in {0,1}^3} w_c(p) z[row(home[p] + c)],  w_c = ((cx ? tx : 1 - tx) (cy ? ty : 1 - ty)) (cz ? tz : 1 - tz),
 *   added in the order c = cx + 2 cy + 4 cz = 0 .. 7.  A corner with no voxel contributes nothing; the weights are NOT renormalised.
 * (16c) csn_point_interp_bwd_f32: the exact adjoint dz[v] = sum_c sum_{p : home[p] = v - c} w_c(p) dy[p], output-stationary over
 *   the voxel rows: per voxel the corners in the order c = 0 .. 7, per corner the points of row(v - c) in CSR order.  EVERY dz row
 *   is written.  No floating-point atomics: two identical calls give the same bits.  One voxel's sum is serial in its G lanes: a
 *   voxel with thousands of points paces its wave (correct for any list length). */
CSN_API int csn_voxel_mean_f32(const float* feats, long long ld_feats, int n_points, const int* vox_ptr, const int* vox_pts,
                       int n_voxels, int channels, float* out, long long ld_out, void* stream);
CSN_API int csn_point_interp_fwd_f32(const float* z, long long ld_z, int n_voxels, const float* coords, const int* home,
                             const int* table, int n_points, int channels, float* y, long long ld_y, void* stream);
CSN_API int csn_point_interp_bwd_f32(const float* dy, long long ld_dy, int n_points, const float* coords, const int* vox_ptr,
                             const int* vox_pts, const int* table, int n_voxels, int channels, float* dz, long long ld_dz,
                             void* stream);

/* ---- (17) kernel maps: the coordinate manager of (14) — packed keys, the coarser level's keys, the offset tables ------------
 * MinkowskiEngine builds its kernel maps in native code; csn_amd.minkowski_conv.build_kernel_map(backend="hip") and
 * csn_amd.minkowski_hrnet.build_pyramid(backend="hip") build theirs here.  The sort and the unique of the keys stay the caller's.
 * PACKED KEY (part of this ABI): a coordinate [b, x, y, z] is the int64
 *   key = b << 48 | (x + 2^15) << 32 | (y + 2^15) << 16 | (z + 2^15),   b in [0, 2^15), x, y, z in [-2^15, 2^15):
 * three 16-bit fields biased by 2^15 below a 15-bit batch field, so that the order of the keys is the lexicographic order of
 * (b, x, y, z) and every valid key is non-negative.
 * STATUS WORD: one int32 on the device, zeroed by the caller, or-ed into by (17a) and (17c) and read by the caller when it likes:
 *   1 a batch index outside [0, 2^15);  2 an x, y or z outside [-2^15, 2^15);  4 an x, y or z that is no multiple of tensor_stride;
 *   8 two neighbours of set_keys equal or descending (a duplicate row, or a set that was not sorted).
 * Nothing is dereferenced through a bad value: a flagged call's outputs are merely not meaningful.
 * Host-side checks before any launch: a NULL pointer (set_rows may be NULL), n < 1, tensor_stride < 1 or step == 0: CSN_E_ARG;
 * kernel_size not in {1, 3, 5}: CSN_E_DIM; a key or coordinate array off 8 bytes, an int32 array or the status word off 4 bytes:
 * CSN_E_PTR.
 * (17a) csn_coord_keys_i64: keys[i] = key(coords[i]) for coords[n][4] int64 (contiguous rows), and the flags 1, 2, 4.  "Multiple of"
 *   in the sense of a floored remainder (-4 is a multiple of 2, -3 is not).
 * (17b) csn_coord_down_i64: down_keys[i] = the key of [b, floor(x / s) s, floor(y / s) s, floor(z / s) s], s = out_tensor_stride.
 *   Floor, not truncation: -1 -> -2 at s = 2.  The batch field is kept.  down_keys may be keys.
 * (17c) csn_kernel_map_i32: set_keys[n_set] ascending, set_rows[n_set] the row number of every sorted key (NULL: its position),
 *   query_keys[n_query] in row order.  With r = kernel_size / 2, o = (ox, oy, oz) in [-r, r]^3 and kidx = (ox + r) + k (oy + r) +
 *   k^2 (oz + r) as in (14): table[kidx][j] = the row of the coordinate "query j + step o" in the set, or -1.  step is signed
 *   (sign x offset step: +ts for the tables indexed by output rows of a convolution, -ts for those indexed by its input rows, the
 *   opposite for the transposed convolution).  The offset is added per field after unpacking: a field that leaves its 16 bits gives
 *   -1, it never carries into the neighbouring field, and the batch field is never touched (offsets cannot cross shapes).  A row
 *   number outside [0, n_set) in set_rows reads as -1.  The same launch raises flag 8.  One thread per query row; per pair (ox, oy) one
 *   lower-bound search and a forward walk over the k keys that differ in z alone; table offsets are 64-bit (kernel_size^3 n_query
 *   may exceed 2^31). */
CSN_API int csn_coord_keys_i64(const long long* coords, int n, int tensor_stride, long long* keys, int* status, void* stream);
CSN_API int csn_coord_down_i64(const long long* keys, int n, int out_tensor_stride, long long* down_keys, void* stream);
CSN_API int csn_kernel_map_i32(const long long* set_keys, const int* set_rows, int n_set, const long long* query_keys, int n_query,
                       int kernel_size, int step, int* table, int* status, void* stream);

/* ---- (18) resident point collections: normalise, augment, collate and key a batch of shapes on the device (MinkowskiNet/lib/
 *           dataset.py:104-126, 221-252, lib/transforms.py:12-89, 195-225, lib/voxelizer.py:34-45) ---------------------------------
 * The reference keeps a category's points in host memory and runs a numpy chain per item and step; csn_amd.minkowski_points keeps
 * them on the device and builds a batch with the entry points below.  Additive to ABI version 17.
 * COLLECTION: points[n_total][3] fp32 (contiguous), offsets[n_shapes + 1] int64 on the DEVICE: shape s is the rows
 *   [offsets[s], offsets[s + 1]), at least one; labels[n_total] int32 or NULL.
 * ITEMS of a batch: idx[n_items] int64 the shape of every item (repeats, any order); params[n_items][9] float64 =
 *   cos, sin, shift_z[3], jitter[3], scale (the cosine and sine of the rotation angle come from the host: no trigonometry here);
 *   out_offsets[n_items] int64 the first output row of every item; bounds[n_items][6] float64 = min x, y, z, max x, y, z.
 * ARITHMETIC: float64 on the fp32 inputs, every operation rounded on its own (no fused multiply-add between a product and an add;
 *   division and square root correctly rounded), sums of three terms as (a + b) + c.  No floating-point atomics: two calls give
 *   the same bits.
 * STATUS WORD, as in (17): one int32 on the device, zeroed by the caller, or-ed into:
 *   1 an item number >= 2^15;  2 a floor(x), floor(y) or floor(z) outside [-2^15, 2^15);  16 a non-finite parameter or coordinate
 *   (then 2 is not raised for that point);  32 a shape index, a CSR offset pair, an output row, a sort position or a voxel number
 *   outside its array: that item or point is SKIPPED (csn_points_bounds_f64 writes zeros for it).  4 and 8 keep their meaning of (17)
 *   and are never raised here.  Nothing is dereferenced through a bad value.  The arrays live on the device, so a bad shape index
 *   cannot be a host-side error here: csn_amd checks its index lists on the host (ValueError) before any launch.
 * Host-side checks before any launch: a NULL pointer (labels may be NULL, labels_out with it), a count < 1, method not 0 or 1,
 *   sigma < 0, clip <= 0, voxel_size <= 0 or any of them NaN: CSN_E_ARG; n_items > 65535 (one grid row per item), n_voxels >
 *   n_points: CSN_E_DIM; an fp32 / int32 array or the status word off 4 bytes, an int64 / float64 array off 8 bytes, coords off 16
 *   bytes: CSN_E_PTR.
 * (18a) csn_points_normalize_f32: per shape c = (sum p) / n and a radius r: method 0 (sphere) r = sqrt(max |p - c|^2), method 1 (box)
 *   r = the diagonal of the bounding box of p - c; r = max(r, 2^-22) (2 eps_fp32); out = fp32((p - c) / r).  out may be points.  One
 *   work-group of 256 threads per shape; the sum is thread t's partial over the rows t, t + 256, ... in that order, then a binary
 *   tree over the 256 partials (partial t + partial t + w, w = 128 .. 1).
 * (18b) csn_points_bounds_f64: per item the minimum and maximum per axis of r = (c x + s z, y, (-s) x + c z): each product rounded,
 *   then one add.  Exact and order-free.  One work-group per item.
 * (18c) csn_points_batch_f32: per point of every item i (grid: chunks of max_points x items), with e = max - min of (18b):
 *   diag = sqrt((ex ex + ey ey) + ez ez);  t = clip((sigma diag) shift_z, -clip, +clip);  q = ((r + t) + jitter) scale;
 *   feats[row] = fp32(q);  coords[row] = [fp32(i), fp32(q / voxel_size)] (a division);  keys[row] = the packed key of (17) of
 *   [i, floor of the three STORED fp32 coordinates], -1 for a point that raised 1, 2 or 16;  labels_out[row] = labels[...] (int64);
 *   row = out_offsets[i] + the point's number inside its shape, inside [0, n_out).  max_points >= the longest shape among the items
 *   (points beyond it are not written).
 * (18d) csn_field_index_i32: skeys[n_points] the ascending keys of a stable sort, order[n_points] its permutation, vid[n_points] the
 *   number of the run of equal keys that position j belongs to (all int64): home[order[j]] = vid[j]; at every run head
 *   vox_ptr[vid[j]] = j and uniq_keys[vid[j]] = skeys[j]; vox_ptr[n_voxels] = n_points; vox_pts[j] = order[j] (int32). */
CSN_API int csn_points_normalize_f32(const float* points, const long long* offsets, int n_shapes, long long n_total, int method,
                             float* out, int* status, void* stream);
CSN_API int csn_points_bounds_f64(const float* points, const long long* offsets, int n_shapes, long long n_total, const long long* idx,
                          const double* params, int n_items, double* bounds, int* status, void* stream);
CSN_API int csn_points_batch_f32(const float* points, const int* labels, const long long* offsets, int n_shapes, long long n_total,
                         const long long* idx, const long long* out_offsets, const double* params, const double* bounds, int n_items,
                         int max_points, double sigma, double clip, double voxel_size, float* coords, float* feats,
                         long long* labels_out, long long* keys, long long n_out, int* status, void* stream);
CSN_API int csn_field_index_i32(const long long* skeys, const long long* order, const long long* vid, int n_points, int n_voxels,
                        int* home, int* vox_ptr, int* vox_pts, long long* uniq_keys, int* status, void* stream);

/* ---- (19) inference: the gather-GEMM with a BatchNorm + residual + ReLU epilogue (MinkowskiNet/models/hrnet.py:124-131 the stem,
 *           :157-161 the branch sums, :308-326 the final transitions; models/modules/resnet_block.py:40-57 the block) ------------
 * In eval mode the statistics of every normalised convolution of the backbone are constants, so (15)'s two launches per
 * convolution — (14) writes z, (15b) reads z (and a residual) back and writes y — need no round trip through memory: ONE launch
 * forms the product of (14) and applies the BatchNorm, the residual and the activation to the accumulators, as (13) does for
 * fc_layer with training == 0.  Additive to ABI version 17.  Everything is POINT-MAJOR fp32 as in (14):
 *   x[n_in][ld_x], table[kv][n_out], w[kv][c_in][c_out] (contiguous), gamma / beta / running_mean / running_var [c_out],
 *   r[n_out][ld_r] (optional: NULL, ld_r then ignored), y[n_out][ld_y].  ld_x, ld_r and ld_y are independent pitches.
 *   acc[j][c] = sum_k x[table[k][j]] W[k]      exactly the sum of csn_sparse_conv_fwd_f32 with bias = NULL: the same contraction
 *                                              order in the same math mode (the same kernel text up to the epilogue)
 *   s[c] = gamma[c] / sqrt(running_var[c] + eps),  t[c] = beta[c] - running_mean[c] s[c]                      (fp32)
 *   y[j][c] = act(acc s + t + r[j][c])         act = ReLU (relu != 0) or the identity; acc s + t is one fused multiply-add
 * A lane owns one column per 32-column block, so s and t are two registers per block formed in the epilogue from the four vectors:
 * no preparation launch, no workspace, no atomics; two identical calls give the same bits.  Nothing but y is written, and y may be
 * a column block of a wider buffer (ld_y > c_out): columns outside [0, c_out) of a row are not written; the same holds for reading
 * x and r.
 * ALIASING: r may be y itself (the same pointer AND ld_r == ld_y): every element is read and then written by the same lane, which
 * is how a sum over branches accumulates in one buffer.  r == y with ld_r != ld_y returns CSN_E_ARG.  Any other overlap of y with
 * r, x, w or the vectors is the caller's error: it is not detected and its result is undefined.
 * Geometry, alignment and window checks and their codes are exactly those of (14), made on the host before any launch, with r (when
 * given) checked like y: n_in, n_out >= 1 (CSN_E_ARG); kv in {1, 27, 125}, c_in % 32 == 0 and c_out % 32 == 0, both in [32, 256]
 * (CSN_E_DIM); every pitch % 4 == 0 (CSN_E_ALIGN), >= its width (CSN_E_ARG), <= 2^20 and rows * pitch * 4 < 2 GiB (CSN_E_DIM); x, w, y,
 * r 16-byte aligned, the table 4-byte (CSN_E_PTR); x, table, w, gamma, beta, running_mean, running_var or y NULL: CSN_E_ARG.
 * Math modes as in (14): mode 0 the exact fp32 matrix instruction, mode 1 bf16x3; modes 2 / 3 run as mode 1 unless
 * csn_set_thread_rows16(1) selects their single-product instances (this is a forward: mode 3 has one).  The launch rule for the
 * column blocks a wave owns and CSN_DEV_SCONV_NB apply as in (14). */
CSN_API int csn_sparse_conv_bn_act_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                   int c_out, const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const float* r, long long ld_r, int relu, float* y,
                                   long long ld_y, void* stream);

/* ---- (20) BatchNorm over row groups: the K + 1 backbone passes of a CSN training step as one (MinkowskiNet/models/hrnet.py:425-454:
 *           the query batch and every key batch is a BatchNorm batch of its own) -------------------------------------------------
 * The rows of a coordinate set are sorted with the batch index leading, so the rows of n_groups batches merged into ONE coordinate
 * set with shifted batch indices are n_groups CONTIGUOUS ranges at every level of the pyramid.  The convolution does not care
 * which batch a row belongs to; only the statistics and the normalisation do.  Additive to ABI version 17.
 *   group_rows[n_groups + 1] int32 on the DEVICE (4-byte aligned: CSN_E_PTR; NULL: CSN_E_ARG): group g is the rows
 *   [group_rows[g], group_rows[g + 1]); n_groups in [1, 8] (< 1: CSN_E_ARG, > 8: CSN_E_DIM).  The offsets live on the device, so the
 *   library cannot read them before the launch: they must start at 0, ascend, end at the row count and leave every group at
 *   least two rows, and the CALLER checks that (csn_amd.minkowski_hrnet.merge_batches does, in its one host read).  Whatever they
 *   hold, no row, tile or part index leaves its array; a row outside every group is neither normalised nor written, a group that
 *   is empty or leaves [0, n_rows] is skipped.
 *   mean / invstd of (20a) and mean[m] / scale[m] of (20b) are [n_groups][channels] fp32.
 * Everything else — layouts, pitches, widths, alignment, math modes, error codes, NULL outputs — is (15)'s.  Training mode only:
 * in eval mode the running statistics do not depend on the group, and (15b) / (19) on the merged rows are the merged pass.
 * No floating-point atomics: every reduction has a fixed order, two identical calls give the same bits.  With n_groups == 1 every
 * output is bit for bit that of (15a) / (15b).
 *
 * (20a) csn_sparse_conv_stats_groups_fwd_f32: z exactly as (15a) on the same map (the same kernel, the same bits); per group g the
 *   mean[g][c] and invstd[g][c] of its rows; the running statistics (either may be NULL) take n_groups updates in group order 0 ..
 *   n_groups - 1, each with that group's mean and its n / (n - 1) variance, as n_groups sequential calls of (15a) would.  Per group:
 *   the whole 32-row tiles of the epilogue's (mean, M2) partials merged as in (15a) — segments of the group's tile list in tile
 *   order, the segments pairwise in a fixed tree, Chan's formula in fp64 — and the <= 31 rows of a tile that a group boundary cuts
 *   re-read from z: their (mean, M2) in fp64, merged after the whole tiles, the piece before them first.  n_out < 2 n_groups:
 *   CSN_E_ARG.  ws: csn_sparse_conv_stats_groups_workspace_bytes(n_out, c_out, n_groups).  Its backward is csn_sparse_conv_bwd_f32.
 * (20b) csn_rows_bn_act_groups_fwd_f32: for row i of group g
 *     y_i = act( sum_{m < n_terms} (gamma_m (z_m,i - mean_m[g]) scale_m[g] + beta_m) + r_i ).
 *   csn_rows_bn_act_groups_bwd_f32: g' = dy [y > 0] read once for all terms; dr = g'; dbeta[m] = sum over ALL rows of g';
 *   dgamma[m] = sum over all rows of g' xhat_m, xhat from the row's own group's statistics;
 *     dz_m,i = gamma_m scale_m[g] (g'_i - mean_g(g') - xhat_m,i mean_g(g' xhat_m)),  the means over group g's rows.
 *   Thread layout as (15b): 64 rows per work-group, a thread owns 4 consecutive channels, 16-byte accesses; a work-group walks the
 *   groups that meet its rows and loads a group's constants when it enters it.  The fp64 chunk sums are cut at the group
 *   boundaries (at most chunks + n_groups - 1 parts), added per group in part order (segments, then the fixed tree), and the groups
 *   in ascending order for dgamma / dbeta.
 *   ws: csn_rows_bn_act_groups_workspace_bytes(n_rows, channels, n_terms, n_groups) bytes (backward only). */
CSN_API long long csn_sparse_conv_stats_groups_workspace_bytes(int n_out, int c_out, int n_groups);
CSN_API int csn_sparse_conv_stats_groups_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                         int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                         float* running_mean, float* running_var, float eps, float momentum, const int* group_rows,
                                         int n_groups, void* ws, long long ws_bytes, void* stream);
CSN_API long long csn_rows_bn_act_groups_workspace_bytes(int n_rows, int channels, int n_terms, int n_groups);
CSN_API int csn_rows_bn_act_groups_fwd_f32(const CsnBnTerms* terms, int n_terms, int n_rows, int channels, const int* group_rows,
                                   int n_groups, const float* r, long long ld_r, int relu, float* y, long long ld_y, void* stream);
CSN_API int csn_rows_bn_act_groups_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const CsnBnTerms* terms,
                                   int n_terms, int n_rows, int channels, const int* group_rows, int n_groups, int relu, float* dr,
                                   long long ld_dr, void* ws, long long ws_bytes, void* stream);

/* ---- (21) kernel-2 stride-2 convolution and its transposed form (MinkowskiNet/models/res16unet.py: conv1p1s2 .. conv4p8s2,
 *           convtr4p16s2 .. convtr7p2s2) ---------------------------------------------------------------------------------------
 * Kernel 2 at stride 2 partitions the fine voxels: every fine row has exactly one parent among the coarse rows and sits in exactly
 * one of its 8 octants.  The caller builds the OCTANT MAP (csn_amd.minkowski_conv.build_octant_map), all int32 on the device:
 *   parent[n_fine]        the coarse row of fine row i
 *   children[8][n_coarse] the fine row in octant k of coarse row j, or -1
 *   order[n_fine]         the fine rows sorted by (octant, row);  seg[9]: octant k is order[seg[k] .. seg[k + 1])
 * DOWN (x[n_fine][c_in] -> y[n_coarse][c_out]):  y[j] = sum_k x[children[k][j]] W[k] + bias
 * UP   (x[n_coarse][c_in] -> y[n_fine][c_out]):  y[i] = x[parent[i]] W[octant[i]] + bias     (one weight per row)
 * Everything is POINT-MAJOR fp32 with pitches as in (14): w[8][c_in][c_out] contiguous (MinkowskiEngine's `kernel`), bias[c_out]
 * may be NULL; columns of a row beyond its width are neither read as data nor written.  A negative index reads as "no voxel"; an
 * index past its array is the caller's error and is never dereferenced (dropped, or caught by the buffer range check); seg is
 * read as a monotone sequence inside [0, n_fine] whatever it holds.
 * Geometry: n_fine, n_coarse >= 1 (CSN_E_ARG); c_in % 32 == 0 and c_out % 32 == 0, both in [32, 256] (CSN_E_DIM); every pitch
 * % 4 == 0 (CSN_E_ALIGN), >= its width (CSN_E_ARG), <= 2^20 and rows * pitch * 4 < 2 GiB (CSN_E_DIM); maps, w, dw and ws 16-byte
 * aligned, the index arrays 4-byte (CSN_E_PTR).  All of this is checked on the host before any launch.  ws (backward only):
 * csn_octant_conv_workspace_bytes(..., up, backward = 1) bytes (CSN_E_WORKSPACE); the forward takes none (backward = 0 returns 0).
 * The gather form (down forward, up dx) is the gather-GEMM of (14) over 8 offsets.  The one-weight form (up forward, down dx) walks
 * `order`: a work-group's tile of <= 128 entries lies inside one segment, the grid is ceil(n_fine / 128) + 7 row groups sized from
 * n_fine alone, every output row is written exactly once and an empty octant costs nothing.
 *   dw[k] = sum_{i : octant[i] = k} in_row(i)^T dy_row(i)   split-K over chunks of `order` cut at the segment bounds, slabs added in
 *                                                           chunk order: work proportional to n_fine; an empty octant's dw is 0
 *   dbias = sum of dy's rows                                fp64 partials of 64-row chunks added in chunk order
 * Each backward output is skipped when its pointer is NULL (its own inputs may then be NULL too).  No floating-point atomics: two
 * identical calls give the same bits.  Math mode 0 runs the products on the exact fp32 matrix instruction, every other mode as
 * bf16x3 whatever csn_set_thread_rows16 says (there are no single-product instances).  Additive to ABI version 17. */
CSN_API long long csn_octant_conv_workspace_bytes(int n_fine, int n_coarse, int c_in, int c_out, int up, int backward);
CSN_API int csn_octant_down_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in, int c_out,
                            const float* w, const float* bias, float* y, long long ld_y, void* stream);
CSN_API int csn_octant_down_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_fine, int n_coarse, int c_in,
                            int c_out, const int* parent, const int* order, const int* seg, const float* w, float* dx,
                            long long ld_dx, float* dw, float* dbias, void* ws, long long ws_bytes, void* stream);
CSN_API int csn_octant_up_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order, const int* seg,
                          int n_fine, int c_in, int c_out, const float* w, const float* bias, float* y, long long ld_y,
                          void* stream);
CSN_API int csn_octant_up_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_fine, int n_coarse, int c_in,
                          int c_out, const int* children, const int* parent, const int* order, const int* seg, const float* w,
                          float* dx, long long ld_dx, float* dw, float* dbias, void* ws, long long ws_bytes, void* stream);

/* ---- (22) octant maps: the coordinate manager of (21) — parent, octant and children by one search per fine row, the rows sorted
 *           by octant ----------------------------------------------------------------------------------------------------------
 * csn_amd.minkowski_conv.build_octant_map(backend="hip") and csn_amd.minkowski_unet.build_unet_pyramid(backend="hip") build the
 * octant map of (21) here, on the PACKED KEY and the STATUS WORD of (17); the sort and the unique of the keys stay the caller's.
 * Additive to ABI version 17.  Two more flags of the status word:
 *   16 a fine row whose parent [b, floor(xyz / 2ts) 2ts] is not in the coarse set (or whose floor leaves [-2^15, 2^15));
 *   32 an entry of `octant` outside [0, 8) handed to (22b).
 * Nothing is dereferenced through a bad value, and no write leaves its array: a flagged call's outputs are merely not meaningful.
 * Host-side checks before any launch: a NULL pointer (fine_sorted and coarse_rows may be NULL), n_fine, n_coarse or n < 1,
 * tensor_stride < 1: CSN_E_ARG; a key array off 8 bytes, an int32 array, the workspace or the status word off 4 bytes: CSN_E_PTR;
 * ws_bytes < csn_octant_order_workspace_bytes(n): CSN_E_WORKSPACE.
 * (22a) csn_octant_partition_i32: fine_keys[n_fine] in row order at tensor_stride ts; coarse_keys[n_coarse] ascending, coarse_rows
 *   [n_coarse] the row number of every sorted key (NULL: its position), as in (17c).  For every fine row i
 *     parent[i] = the coarse row of [b, floor(xyz / 2ts) 2ts], or -1 (flag 16; no children entry is written for it);
 *     octant[i] = ox + 2 oy + 4 oz, o = (xyz - floor(xyz / 2ts) 2ts) / ts   (always in [0, 8));
 *     children[octant[i]][parent[i]] = i;   every other entry of children[8][n_coarse] is -1: the entry point fills the array.
 *   Floor, not truncation (-1 -> -2 at ts = 1), per field after unpacking; the batch field is never touched.  One lower-bound search
 *   per fine row; offsets into children are 64-bit.  A row number outside [0, n_coarse) in coarse_rows reads as "no parent".  With
 *   unique fine rows every (octant, parent) slot has one writer at most: no atomics on data, the same integers on every call.
 *   Duplicate fine rows are the caller's to exclude: fine_sorted[n_fine], the fine keys ascending, has its neighbours checked in the
 *   same launch (flag 8, like those of coarse_keys); NULL where a (17c) call on that set has checked them already.
 * (22b) csn_octant_order_i32: order[n] = the rows sorted by (octant, row), seg[9] with octant k at order[seg[k] .. seg[k + 1]): the
 *   integers of a stable sort of octant[n] and of the running sum of its histogram.  A stable counting sort in three launches over
 *   tiles of 256 rows: counts per tile and octant from wave ballots; one work-group scans the counts octant by octant, 256 tiles
 *   per pass, and writes seg; a scatter in which a row's rank inside its tile is the population count of its octant's ballot below
 *   its lane plus the counts of the waves before its own.  No position comes from an atomic counter.  An entry outside [0, 8)
 *   (which (22a) never writes) is dropped and flagged 32: seg[8] is then the number of rows kept and order[seg[8] .. n) is left as
 *   it was.  ws: csn_octant_order_workspace_bytes(n) = 8 ceil(n / 256) int32 (0 for n < 1). */
CSN_API int csn_octant_partition_i32(const long long* fine_keys, const long long* fine_sorted, int n_fine, int tensor_stride,
                             const long long* coarse_keys, const int* coarse_rows, int n_coarse, int* parent, int* octant,
                             int* children, int* status, void* stream);
CSN_API long long csn_octant_order_workspace_bytes(int n);
CSN_API int csn_octant_order_i32(const int* octant, int n, int* order, int* seg, void* ws, long long ws_bytes, int* status,
                         void* stream);

/* ---- (23) inference: the octant convolutions of (21) with the BatchNorm + residual + ReLU epilogue of (19) (MinkowskiNet/models/
 *           res16unet.py: conv{n}p{ts}s2 + bn{n} + relu, convtr{n}p{ts}s2 + bntr{n} + relu) ------------------------------------------
 * In eval mode a Res16UNet's eight resolution changes need no round trip of z through memory either: ONE launch forms the product
 * of (21) and applies the BatchNorm on its running statistics, an optional residual and the activation to the accumulators.
 * Additive to ABI version 17.  The map arguments are (21)'s without bias, the tail is (19)'s:
 *   DOWN  acc[j] = sum_k x[children[k][j]] W[k]      y[n_coarse][ld_y], r[n_coarse][ld_r]
 *   UP    acc[i] = x[parent[i]] W[octant[i]]         y[n_fine][ld_y],   r[n_fine][ld_r]
 *   s[c] = gamma[c] / sqrt(running_var[c] + eps),  t[c] = beta[c] - running_mean[c] s[c]                      (fp32)
 *   y[.][c] = act(acc s + t + r[.][c])               act = ReLU (relu != 0) or the identity; acc s + t is one fused multiply-add
 * acc is exactly the sum of csn_octant_down_fwd_f32 / csn_octant_up_fwd_f32 with bias = NULL in the same math mode: the same
 * contraction loop text, the same order.  s and t are formed per column block in the epilogue from the four vectors: no
 * preparation launch, no workspace, no atomics; two identical calls give the same bits.  Nothing but y is written; x, r and y may
 * be column blocks of wider buffers (independent pitches).  DOWN is (19)'s kernel over a table of 8 offsets: a coarse row without
 * children has acc = 0 and gives act(t + r).  UP are kernels of their own around (21)'s one-weight loop; its index rules hold: a
 * destination order[r] outside [0, n_fine) is dropped, a parent past n_coarse reads as no voxel (acc = 0), seg is read as a
 * monotone sequence inside [0, n_fine], y and r go through buffer descriptors with the range check, every output row is written
 * exactly once.
 * ALIASING as in (19): r may be y itself (the same pointer AND ld_r == ld_y), every element read and then written by the same lane;
 * r == y with ld_r != ld_y returns CSN_E_ARG; any other overlap is the caller's error.
 * Host-side checks before any launch — exactly (21)'s codes, with r (when given; NULL: ld_r ignored) checked like y as in (19):
 * x, an index array, w, a vector or y NULL, n_fine or n_coarse < 1: CSN_E_ARG; c_in % 32 == 0 and c_out % 32 == 0, both in [32, 256]
 * (CSN_E_DIM); every pitch % 4 == 0 (CSN_E_ALIGN), >= its width (CSN_E_ARG), <= 2^20 and rows * pitch * 4 < 2 GiB (CSN_E_DIM); x, w,
 * y, r 16-byte aligned, the index arrays 4-byte (CSN_E_PTR).
 * Math modes as in (21): mode 0 the exact fp32 matrix instruction, every other mode bf16x3 whatever csn_set_thread_rows16 says.
 * The launch rule for the column blocks a wave owns and CSN_DEV_SCONV_NB apply as in (21). */
CSN_API int csn_octant_down_bn_act_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in,
                                   int c_out, const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const float* r, long long ld_r, int relu, float* y,
                                   long long ld_y, void* stream);
CSN_API int csn_octant_up_bn_act_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order,
                                 const int* seg, int n_fine, int c_in, int c_out, const float* w, const float* gamma,
                                 const float* beta, const float* running_mean, const float* running_var, float eps, const float* r,
                                 long long ld_r, int relu, float* y, long long ld_y, void* stream);

/* ---- (24) inference: the launch of (19) on 16-bit maps (the maps between the launches of HRNetBackbone's inference graph) ---------
 * Under csn_set_thread_rows16(1) in math mode 2 / 3, (19) rounds every gathered value to bf16 / fp16 as the first thing it does with
 * it, yet the map it gathers from was written and is read as fp32.  Here x, r and y may each be rows of the mode's OWN 16-bit type
 * (mode 2: bf16, mode 3: fp16): gather bytes, map writes and residual reads halve, the conversions of x leave the contraction loop.
 * Additive to ABI version 17.  The arguments are (19)'s with a type flag beside each map:
 *   x16 / r16 / y16   0: fp32 rows, 1: 16-bit rows.  Any other value: CSN_E_ARG.  ld_x / ld_r / ld_y count ELEMENTS of the map's own
 *                     type.  table, w and the four vectors are as in (19) (w is fp32 and rounded when it is staged, as there).
 *   acc, s, t         as in (19); y[j][c] = act(acc s + t + r[j][c]), stored as fp32 (y16 == 0) or rounded ONCE to the 16-bit type
 *                     (nearest even, as a CPU cast).  An fp16 store that overflows is a plain conversion (inf), not a clamp.
 * EXACTNESS: a 16-bit map changes where a value is rounded, not which product is formed.  Given the same representable inputs the
 * call is bit-identical to csn_sparse_conv_bn_act_fwd_f32 under csn_set_thread_rows16(1) in the same math mode, its fp32 output
 * rounded once when y16 == 1: a 16-bit x holds exactly what (19) would have rounded its fp32 value to, a 16-bit r converts to fp32
 * exactly, w is rounded when staged as there, and the contraction walks the same (offset, 32-channel step) sequence under the same
 * launch rule for the column blocks (CSN_DEV_SCONV_NB included) — the accumulators are the same bits.  All three flags 0 is allowed
 * and gives the bits of (19).  No workspace, no atomics; two identical calls give the same bits.  Nothing but y is written; x, r and
 * y may be column blocks of wider buffers of their own type.
 * Requires math mode 2 or 3 AND csn_get_thread_rows16() == 1, otherwise CSN_E_ARG: there are no bf16x3 / fp32 instances (16-bit maps
 * under those modes would throw away what they pay for).
 * ALIASING: r may be y itself — the same pointer AND r16 == y16 AND ld_r == ld_y — every element read and then written by the same
 * lane; r == y with another type or pitch returns CSN_E_ARG.  Any other overlap is the caller's error, as in (19).
 * Host-side checks before any launch: (19)'s for NULLs, n_in, n_out, kv in {1, 27, 125} and the widths, and for every fp32 map
 * (pitch % 4 CSN_E_ALIGN, >= width CSN_E_ARG, <= 2^20 and rows * pitch * 4 < 2 GiB CSN_E_DIM).  A 16-bit map needs pitch % 8 == 0
 * (CSN_E_ALIGN), pitch >= width (CSN_E_ARG), pitch <= 2^20 and rows * pitch * 2 < 2 GiB (CSN_E_DIM).  x, w, y, r 16-byte aligned
 * whatever their type, the table 4-byte (CSN_E_PTR). */
CSN_API int csn_sparse_conv_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_in, const int* table, int n_out, int kv,
                                   int c_in, int c_out, const float* w, const float* gamma, const float* beta,
                                   const float* running_mean, const float* running_var, float eps, const void* r, int r16,
                                   long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream);

/* ---- (25) inference: the launches of (23) as ONE 16-bit product on 16-bit maps (the maps between the launches of a Res16UNet's
 *           inference graph) ------------------------------------------------------------------------------------------------------
 * (23) runs the octant products as bf16x3 on fp32 maps whatever csn_set_thread_rows16 says.  Here they are the single product of
 * (14) / (24): every operand rounded once to the math mode's 16-bit type, ONE matrix instruction per operand pair, and x, r and y
 * may each be rows of that type (mode 2: bf16, mode 3: fp16).  Additive to ABI version 17.  The arguments are (23)'s with (24)'s type
 * flag beside each map:
 *   x16 / r16 / y16   0: fp32 rows, 1: 16-bit rows.  Any other value: CSN_E_ARG.  ld_x / ld_r / ld_y count ELEMENTS of the map's own
 *                     type.  The index arrays, w and the four vectors are as in (23) (w is fp32 and rounded when it is staged).
 *   DOWN  acc[j] = sum_k x[children[k][j]] W[k]      y[n_coarse][ld_y], r[n_coarse][ld_r]
 *   UP    acc[i] = x[parent[i]] W[octant[i]]         y[n_fine][ld_y],   r[n_fine][ld_r]
 *   s, t              as in (23); y[.][c] = act(acc s + t + r[.][c]) with acc s + t one fused multiply-add, stored as fp32
 *                     (y16 == 0) or rounded ONCE to the 16-bit type (nearest even, as a CPU cast).  An fp16 store that overflows is
 *                     a plain conversion (inf), not a clamp.
 * DOWN is (24)'s kernel over children as a table of 8 offsets (the entry point of (24) itself refuses kv == 8, and that stays): the
 * same column-block rule, a coarse row without children has acc = 0 and gives act(t + r).  UP are kernels of their own around (21)'s
 * one-weight walk — tiles of at most 128 entries of order cut at the segment bounds, one W[k] per tile, ceil(n_fine / 128) + 7 row
 * groups, (21)'s rule for the column blocks a wave owns, CSN_DEV_SCONV_NB included.  (23)'s index rules hold unchanged: a destination
 * order[r] outside [0, n_fine) is dropped, a parent past n_coarse reads as no voxel (acc = 0), seg is read as a monotone sequence
 * inside [0, n_fine], x, y and r go through buffer descriptors sized in bytes of the map's own type, every output row is written
 * exactly once.
 * EXACTNESS: with all three flags 0 UP gives, element for element, the value DOWN gives over the table t[k][i] = parent[i] where
 * octant[i] == k and -1 elsewhere (the other seven offsets add exact zeros).  A 16-bit map changes where a value is rounded, not which
 * product is formed: given the same representable inputs a call is bit-identical to the all-flags-0 call, its output rounded once
 * when y16 == 1.  No workspace, no atomics; two identical calls give the same bits.  Nothing but y is written; x, r and y may be
 * column blocks of wider buffers of their own type.
 * Requires math mode 2 or 3 AND csn_get_thread_rows16() == 1, otherwise CSN_E_ARG.  All three flags 0 is allowed: the single-product
 * octant product on fp32 maps.
 * ALIASING as in (24): r may be y itself — the same pointer AND r16 == y16 AND ld_r == ld_y; r == y with another type or pitch returns
 * CSN_E_ARG.  Any other overlap is the caller's error.
 * Host-side checks before any launch: (23)'s for NULLs, n_fine, n_coarse and the widths, and for every fp32 map (pitch % 4
 * CSN_E_ALIGN, >= width CSN_E_ARG, <= 2^20 and rows * pitch * 4 < 2 GiB CSN_E_DIM).  A 16-bit map needs pitch % 8 == 0 (CSN_E_ALIGN),
 * pitch >= width (CSN_E_ARG), pitch <= 2^20 and rows * pitch * 2 < 2 GiB (CSN_E_DIM).  x, w, y, r 16-byte aligned whatever their
 * type, the index arrays 4-byte (CSN_E_PTR). */
CSN_API int csn_octant_down_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_fine, const int* children, int n_coarse,
                                   int c_in, int c_out, const float* w, const float* gamma, const float* beta,
                                   const float* running_mean, const float* running_var, float eps, const void* r, int r16,
                                   long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream);
CSN_API int csn_octant_up_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_coarse, const int* parent, const int* order,
                                 const int* seg, int n_fine, int c_in, int c_out, const float* w, const float* gamma,
                                 const float* beta, const float* running_mean, const float* running_var, float eps, const void* r,
                                 int r16, long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream);

/* ---- (26) training: the octant products of (21) with the BatchNorm statistics epilogue of (15a) (MinkowskiNet/models/res16unet.py:
 * conv{1..4}p*s2 + bn{1..4}, convtr{4..7}p*s2 + bntr{4..7}) ---------------------------------------------------------------------
 * Every resolution change of a Res16UNet is followed by a BatchNorm.  Here the product's epilogue forms the statistics of its
 * batch, so that (15b) normalises, activates and takes the whole BatchNorm gradient in one launch each way, as for the kernel-3
 * convolutions.  Additive to ABI version 17.  The map arguments are (21)'s without bias, the tail is (15a)'s:
 *   z                 exactly what csn_octant_down_fwd_f32 / csn_octant_up_fwd_f32 write with bias = NULL in the same math mode:
 *                     the same bits, under the same launch rule for the column blocks a wave owns, CSN_DEV_SCONV_NB included.
 *   mean, invstd      [c_out], of the BatchNorm batch z: n_coarse rows (down), n_fine rows (up); invstd = 1 / sqrt(biased variance
 *                     + eps).  running_mean / running_var [c_out] (either may be NULL) are updated in place with `momentum`,
 *                     running_var with the n / (n - 1) variance, as in (15a).
 * DOWN is (15a)'s kernel over children as a table of 8 offsets.  UP are kernels of their own around (21)'s one-weight loop: a
 * work-group's tile of <= 128 entries of `order` lies inside ONE octant segment, so a wave's tile holds 0 to 32 rows anywhere in
 * the grid; the wave stores the (mean, M2) of its rows WITH ITS OWN ROW COUNT, a row group without a span stores zero counts, and
 * the merge takes every tile's count from there (Chan's formula in fp64, tiles in grid order, 64 segments per column merged pairwise
 * in a fixed tree).  An empty octant and an empty tile contribute nothing.  (21)'s index rules hold: a destination outside
 * [0, n_fine) is dropped — and not counted —, a parent past n_coarse reads zeros.  No floating-point atomics: two identical calls
 * give the same bits.
 * ws: csn_octant_stats_workspace_bytes(n_fine, n_coarse, c_out, up) bytes (CSN_E_WORKSPACE; 0 for arguments (21) refuses).
 * Host-side checks before any launch — (21)'s codes for NULLs, n_fine, n_coarse, the widths, pitches, windows and alignment (ws
 * 16-byte aligned); a BatchNorm batch of fewer than 2 rows (n_coarse for down, n_fine for up): CSN_E_ARG (no variance).
 * Math modes as in (21): mode 0 the exact fp32 matrix instruction, every other mode bf16x3 whatever csn_set_thread_rows16 says.
 * The backward is csn_octant_down_bwd_f32 / csn_octant_up_bwd_f32 with dbias = NULL (the statistics are taken up by (15b)'s dz). */
CSN_API long long csn_octant_stats_workspace_bytes(int n_fine, int n_coarse, int c_out, int up);
CSN_API int csn_octant_down_stats_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in,
                                  int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                  float* running_mean, float* running_var, float eps, float momentum, void* ws, long long ws_bytes,
                                  void* stream);
CSN_API int csn_octant_up_stats_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order,
                                const int* seg, int n_fine, int c_in, int c_out, const float* w, float* z, long long ld_z,
                                float* mean, float* invstd, float* running_mean, float* running_var, float eps, float momentum,
                                void* ws, long long ws_bytes, void* stream);

/* ---- (27) training: (15a) over a concatenation that is never formed (MinkowskiNet/models/res16unet.py: block5 .. block8 read
 * me.cat(up, skip); a block that reads more than 256 columns) -------------------------------------------------------------------
 *   z = sum_{m < n_parts} gather-GEMM(x_m, table, W[:, c0_m : c1_m]),  c0_m = sum_{i < m} c_in[i], c1_m = c0_m + c_in[m]
 * for n_parts in [1, 4] maps x_m[n_in][ld_x[m]] of c_in[m] columns (each a multiple of 32 in [32, 256]; the parts may be column
 * blocks of one wider buffer) and ONE contiguous kernel w[kv][sum c_in][c_out], the module's parameter: part m's weights are rows
 * [c0_m, c1_m) of every W[k], reached by a base offset with the unchanged row pitch c_out — no weight is copied or cut.  mean,
 * invstd and the running statistics of z are (15a)'s, formed by the epilogue of the launch that completes z: no pass of their own
 * over z.  Additive to ABI version 17.
 * A chain of one launch per part: the first writes z, each later one adds its product to z in place (every element read and then
 * written by the same lane), the last also forms the tiles' (mean, M2); then (15a)'s merge.  z therefore must not overlap any x_m.
 * With one part the call is (15a) and gives its bits.  kv in {1, 27} (CSN_E_DIM), table[kv][n_out] as in (14) at stride 1 or 2.
 * Host-side checks before any launch: parts NULL or n_parts outside [1, 4] CSN_E_ARG; a width outside the rule or c_out outside
 * (14)'s CSN_E_DIM; every map's pitch and window as in (14); x_m, w, z, ws 16-byte aligned (CSN_E_PTR); n_out < 2 CSN_E_ARG;
 * ws: csn_sparse_conv_cat_stats_workspace_bytes(n_out, c_out) bytes (CSN_E_WORKSPACE).
 * Math modes and csn_set_thread_rows16 as in (15a).  The backward is csn_sparse_conv_bwd_f32 per part on that part's slice of w. */
typedef struct CsnCatParts {
  const float* x[4];
  long long ld_x[4];
  int c_in[4];
} CsnCatParts;
CSN_API long long csn_sparse_conv_cat_stats_workspace_bytes(int n_out, int c_out);
CSN_API int csn_sparse_conv_cat_stats_fwd_f32(const CsnCatParts* parts, int n_parts, int n_in, const int* table, int n_out, int kv,
                                      int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                      float* running_mean, float* running_var, float eps, float momentum, void* ws,
                                      long long ws_bytes, void* stream);

/* ---- (28) training: the fused tail of (15) and the backward of (14) on bf16 activation maps (the ReLU outputs between the layers of
 * HRNetBackbone's training graph) ------------------------------------------------------------------------------------------------
 * The training counterpart of (24).  In math mode 2 behind csn_set_thread_rows16 a convolution rounds its gathered input to bf16
 * before the product and its weight gradient rounds the same map again; a ReLU output y that only such launches read can therefore
 * be STORED as bf16 rows: the products are the same, y's one write and three reads (the next convolution, its weight gradient, the
 * ReLU mask of (15b)'s backward) move half the bytes.  z, mean / invstd and every gradient map (dy, dz, dx, dr) stay fp32.
 * Additive to ABI version 17.  Each entry point is an existing one with a TYPE FLAG beside the map that may be bf16 (0: fp32 rows as
 * ever — the call IS the existing one —, 1: bf16 rows; anything else CSN_E_ARG); a bf16 map's pitch counts ELEMENTS:
 *   csn_sparse_conv_stats_fwd_t16   (15a) with x / x16.  z, mean, invstd and the running statistics are the bits of
 *                                   csn_sparse_conv_stats_fwd_f32 on the same values held as fp32 (the same column-block rule,
 *                                   offset list, matrix instructions and statistics epilogue).
 *   csn_rows_bn_act_fwd_t16         (15b) forward with r / r16 and y / y16.  v is formed as there; a bf16 y is to_bf16(v), ONE
 *                                   rounding to nearest even; a bf16 r is widened exactly.
 *   csn_rows_bn_act_bwd_t16         (15b) backward with y / y16: g' = dy [y > 0] on the stored value (round(relu(v)) > 0 where the
 *                                   forward stored bf16); dr, dz, dgamma, dbeta as there, the same fp64 sums in the same order.
 *   csn_sparse_conv_bwd_t16         (14) backward with x / x16: dw is the bits of csn_sparse_conv_bwd_f32 in mode 2 on the same values
 *                                   held as fp32 (the same 16-row steps, skipped steps, split-K chunks and slab reduction); dx and
 *                                   dbias do not read x and are (14)'s launches.
 * Host-side checks before any launch: the thread's math mode is not 2, or csn_set_thread_rows16 is off, CSN_E_ARG (a bf16 map
 * under bf16x3 or fp32 would throw away what it pays for; fp16 runs its backward in bf16 and would round an fp16 map twice); a
 * bf16 map: pitch >= width (CSN_E_ARG), pitch % 8 == 0 (CSN_E_ALIGN), pitch <= 2^20 and rows * pitch * 2 bytes inside the 2 GiB
 * window (CSN_E_DIM), base 16-byte aligned (CSN_E_PTR); everything else as in (14) / (15): widths multiples of 32 in [32, 256],
 * n_out >= 2 for the statistics, the workspaces of csn_sparse_conv_stats_workspace_bytes, csn_rows_bn_act_workspace_bytes and
 * csn_sparse_conv_workspace_bytes(.., 1).  The whole map is one BatchNorm batch: no row-group form. */
CSN_API int csn_sparse_conv_stats_fwd_t16(const void* x, int x16, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                  int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                  float* running_mean, float* running_var, float eps, float momentum, void* ws, long long ws_bytes,
                                  void* stream);
CSN_API int csn_rows_bn_act_fwd_t16(const CsnBnTerms* terms, int n_terms, int n_rows, int channels, int training, float eps,
                            const void* r, int r16, long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream);
CSN_API int csn_rows_bn_act_bwd_t16(const float* dy, long long ld_dy, const void* y, int y16, long long ld_y, const CsnBnTerms* terms,
                            int n_terms, int n_rows, int channels, int training, float eps, int relu, float* dr, long long ld_dr,
                            void* ws, long long ws_bytes, void* stream);
CSN_API int csn_sparse_conv_bwd_t16(const float* dy, long long ld_dy, const void* x, int x16, long long ld_x, int n_in, int n_out, int kv,
                            int c_in, int c_out, const int* fwd_table, const int* bwd_table, const float* w, float* dx,
                            long long ld_dx, float* dw, float* dbias, void* ws, long long ws_bytes, void* stream);

/* ---- DEVELOPMENT SECTION -------------------------------------------------------------------------------------------------
 * Kernel-selection switches for A/B timing and for the equality tests between two kernel forms of one product.  They are
 * PROCESS-wide, not thread-safe, change no result beyond fp32 rounding and are not part of the drop-in surface: a product
 * build leaves every key at its default.  csn_dev_set returns the previous value (CSN_E_ARG for an unknown key or a value
 * that the key does not take; the setting is then unchanged).
 *   CSN_DEV_BIG_TILES   1   256 x 256 GEMM tiles where the output fills them (0: 128 x 128 tiles everywhere)
 *   CSN_DEV_WIDE_GEMM   1   sixteen-wave form of the 256 x 256 tiles in the bf16x3 mode (0 off, 2: the one-plane modes too)
 *   CSN_DEV_WIDE_FORMS  7   bit set of the product forms that take it: 1 plain, 2 tile-plane B (dV / dK), 4 weight gradients
 *   CSN_DEV_WX          9   bit set for the K = 256 weight products of the bf16x3 mode: 1 projections, dCtx and out-projection +
 *                           LayerNorm on the weight-stationary streaming kernel (0: the tiled GEMM kernels); 4 out-projection +
 *                           LayerNorm back on the tiled kernel; 8 LayerNorm backward fused into the dCtx stream.  Any other bit:
 *                           CSN_E_ARG (2 and 16..128 were the staggered wave halves and timing-only ablations of round 4; removed) */
#define CSN_DEV_BIG_TILES 0
#define CSN_DEV_WIDE_GEMM 1
#define CSN_DEV_WIDE_FORMS 2
#define CSN_DEV_WX 3
/* (key 4 was the 32-queries-per-wave attention forward of round 4: measured 25 % slower, removed; profiles/README.md) */
#define CSN_DEV_LNB_GROUP 5 /* default 0; G > 0: csn_outproj_ln_bwd_f32 runs its LayerNorm backward and its dCtx product over groups
                               of G evaluations (bf16x3, streaming dCtx; the same results) */
/* (key 6 was the output-stationary dV / dK stream of round 5: the GEMM route is as fast over the step; profiles/r5_dkv_stream.txt) */
#define CSN_DEV_SCONV_NB 7  /* default 0: csn_sparse_conv_* choose the 32-column blocks a wave owns by their launch rule; 1..4 pins
                               them (capped at c / 32) so that every kernel instance can be reached at any size — the same sums */
#define CSN_DEV_KV_SAME 8   /* default 1: csn_block_attn_bwd_dq_f32 with probs_tiles = 3 and k == v (bf16x3, d_head = 256) requests
                               every key tile once for both LDS images (0: once per image) — the same bits.  Other values: CSN_E_ARG */
#define CSN_DEV_ATTN_WG64 9 /* default 1: csn_block_attn_bwd_dq_f32 with probs_tiles = 3 and k == v (tile planes, bf16x3, d_head = 256)
                               launches four waves and 64 queries per work-group on ONE LDS tile image, two work-groups per CU
                               (0: eight waves and 128 queries, as CSN_DEV_KV_SAME says) — the same bits.  Other values: CSN_E_ARG */
#define CSN_DEV_ATTN_WG64_LAUNCHES 10 /* read-only (csn_dev_set: CSN_E_ARG): launches that took the 64-query instance so far */
CSN_API int csn_dev_set(int key, int value);
CSN_API int csn_dev_get(int key);

#ifdef __cplusplus
}
#endif
#endif /* CSN_HIP_H */
