// Internal launch interface between the kernel translation units and the C-ABI (csn_capi.hip).
#pragma once
#include "csn_common.h"

struct CsnGemmArgs {
  CsnOperand A, B, C;
  int M, N, K;
  int n0, n1;        // blockIdx.z = (z2 * n1 + z1) * n0 + z0
  int k_chunk;       // > 0: this z0 contracts only k in [0, min(k_chunk, K - z0*k_chunk)); the operand
                     //      strides s0 carry the matching offsets (split-K over the point index)
  float alpha;
  int div_rows;      // output rows m < div_rows are divided by div_val (query scaling, csa_models.py:139)
  float div_val;
  int accumulate;    // C += result
  const int* eval_ids;   // optional: blockIdx.z's slowest index z2 -> evaluation id, applied before the operands' idx2
  int batch;             // number of batch items z (filled in by the launcher)
  // grouped accumulation (256 x 256 bf16x3 kernel): the slowest batch index z2 counts GROUPS; group g contracts the items
  // grp_items[grp_off[g] .. grp_off[g+1]) one after the other into the same accumulators (A and B are addressed by the item,
  // C by the group's first item) and writes once — evaluations that share an output slot need no read-modify-write passes
  const int* grp_off = nullptr;
  const int* grp_items = nullptr;
  // ragged batches (varlen attention backward): per-item column / contraction counts, indexed by the slowest batch index
  // z2 (after eval_ids); N and K above are then the maxima that size the grid.  n_arr[z] is rounded up to 4; k_arr[z] % 4 == 0.
  const int* n_arr = nullptr;
  const int* k_arr = nullptr;
  // ragged last block (block attention backward): the LAST item of the fastest batch index z0 (= the last attention block)
  // has n_last columns and k_last contraction steps (0 = like the others)
  int n_last = 0, k_last = 0;
};

int csn_launch_gemm_f32(const CsnGemmArgs& a, int b_is_nk, int batch, hipStream_t st);
int csn_launch_gemm_bf16x3(const CsnGemmArgs& a, int b_is_nk, int batch, int mode, hipStream_t st);   // gemm_bf16x3.hip; mode 1 bf16x3, 2 bf16, 3 fp16
int csn_gemm_tile_major_planes(int M, int N);         // 1: B.planes == 3 (tile-major tile planes, CsnAttnArgs::sc_layout) is available for an M x N output
int csn_gemm_bf16x3_big_tiles(int M, int N);          // 1: an M x N output takes the 256 x 256 kernel (grouped accumulation available)
int csn_launch_slab_reduce(const float* slab, float* out, int n_slabs, long long n, float alpha, int accumulate,
                           hipStream_t st);

// ---- weight-stationary streaming products, K = 256, bf16x3 (wx_stream.hip) ---------------------------------
struct CsnWxArgs {
  const float* w;                                         // [n_sets * 256][256] row-major
  const float* x;  long long x_item_stride;  int ldx;     // [item][256][ldx] fp32
  void* out;  long long out_item_stride;  int ldo;        // fp32 [item][n_sets * 256][ldo], or bf16 tile planes (strides in 16-bit elements)
  int n_items, n_points, n_sets;
  int div_rows;  float div_val;  float div_rcp;  int div_exact;   // rows < div_rows are divided by div_val (exact as * div_rcp when it is a power of two)
  int tb;                                                 // tile planes: points per attention block
  // out_mode 3 — out-projection + fc dropout + residual + LayerNorm (csa_models.py:115-118): x = Ctx^T, w = W_fc, out = xhat
  const float* res = nullptr;  long long res_shape_stride = 0;  const int* res_index = nullptr;   // residual x[shape][256][ldo]
  float* rstd = nullptr;                                  // [item][n_points]
  float eps = 0.f, dropout_p = 0.f;  unsigned long long seed = 0;
  float* sum_ws = nullptr;  int sum_slots = 0;            // optional [item][sum_slots][256]: per-stream sums over points of xhat
  // out_mode 4 — Q | K | V in one pass over x: the first n_f32 row sets leave as fp32 maps, the others as tile planes through `out`
  float* out_f32 = nullptr;  long long out_f32_item_stride = 0;  int ldo_f32 = 0;  int n_f32 = 0;
};
// "this geometry is not taken by the streaming kernel": an INTERNAL return value of the csn_launch_wx* launchers, distinct from
// every CSN_E_* status of the C ABI — the caller falls through to the tiled kernels and never hands it to the user
constexpr int CSN_NOT_TAKEN = -1000;
extern int csn_gemm_big_tiles, csn_gemm_wide, csn_gemm_wide_set, csn_dev_wx, csn_dev_lnb_group;   // development switches (csn_dev_set)
bool csn_wx_geometry_takes(int n_items, int n_points, int n_sets);   // ... and this launch geometry (else CSN_NOT_TAKEN)
bool csn_wx_takes(int rows, int k);                       // this product shape runs on the streaming kernel
int csn_launch_wx(const CsnWxArgs& a, int out_mode /* 0 fp32, 2 tile planes, 3 LayerNorm, 4 fp32 + tile planes */, hipStream_t st);
int csn_wx_ln_sum_slots(int n_items, int n_points);      // out_mode 3: sum_slots the launch will use (sum_ws = n_items * slots * 256 floats)
int csn_launch_wx_ln_sums(const float* ws, float* out, int n_items, int n_points, hipStream_t st);   // out[item][256] from sum_ws

// ---- folded projections: x as tile planes, small transposes (fold.hip) -------------------------------------
struct CsnTilePlanesArgs {
  const float* x;  long long x_item_stride;  int ldx;     // [item][rows][ldx] fp32
  short* out;  long long out_item_stride;  int ldo;       // bf16 tile planes [item][rows][ldo] (strides in 16-bit elements)
  int n_items, rows, n_points;
  int tb;                                                 // points per attention block
};
int csn_launch_tile_planes(const CsnTilePlanesArgs& a, hipStream_t st);
struct CsnTransposeArgs {
  const float* src[3];  float* dst[3];                    // n contiguous row-major [rows][cols] matrices -> [cols][rows]
  int n, rows, cols;
};
int csn_launch_transpose_f32(const CsnTransposeArgs& a, hipStream_t st);

// ---- fused block attention (attn_f32.hip) -----------------------------------------------------
struct CsnAttnArgs {
  // channel-major projected features, one slab of [H*d][ld] per shape
  const float* q;  const float* k;  const float* v;     // forward: Qs^T, K^T, V^T ; backward: dO^T(=dCtx^T), V^T, K^T
  long long q_shape_stride, kv_shape_stride;             // elements between consecutive shapes
  const int* q_index; const int* kv_index;               // evaluation e -> shape slot (nullptr: identity)
  int ld;                                                // points per row (leading dimension)
  float* out;        long long out_eval_stride;          // forward: Ctx^T[e][H*d][ld] ; backward: dQs^T[e][H*d][ld]
  float* scores;                                         // S^T / P^T  [e][h][blk][T][Tp]   (may be null in forward)
  float* dscores;                                        // backward: dS^T, same geometry
  float* lse;                                            // [e][h][n_blocks*T]
  float* delta;                                          // backward: rowsum(dO*O) [e][h][n_blocks*T], computed by the kernel
  const float* ctx;                                      // backward: O^T = Ctx^T [e][H*d][ld] of the forward (for delta)
  int E, H, T, Tp, n_blocks;
  float rescale_threshold;
  const int* eval_ids;                                   // launch z -> evaluation id (nullptr: identity); E = launch size
  const int* grp_off;                                    // backward, optional: E counts groups; group g = eval_ids[grp_off[g] .. grp_off[g+1])
  const int* out_index;                                  // evaluation -> output slot (nullptr: the evaluation itself)
  int accumulate;                                        // out += result (several evaluations share an output slot)
  float dropout_p;                                       // attention-probability dropout (csa_models.py:141); 0 = off
  unsigned long long seed;
  // bf16x3 kernels only.  kv_planes != 0: k and v point into a "tile plane" tensor written by the projection
  // (bf16; per row and block 16 tiles of [hi: 32 keys | lo: 32 keys], block pitch 1024, row pitch kv_ld = n_blocks * 1024);
  // kv_shape_stride then counts bf16 elements.  r_planes / *_plane_stride: reserved.
  int r_planes, kv_planes;
  long long r_plane_stride, kv_plane_stride;
  int kv_ld;
  int Tq;                                                // queries per block (0: = T); T counts the keys
  int ld_kv;                                             // leading dimension of the fp32 K/V maps (0: = ld)
  int sc_tiles;                                          // backward (bf16x3): P and dS leave as bf16 tile planes [query][tile: hi 32 | lo 32]
  // ragged batches (n_blocks = 1): per-evaluation query / key counts (device arrays; null = Tq / T for every evaluation).
  // Tq and T are then the maxima: they size the grid, the score pitch and the buffers; tq_arr[e] % 4 == 0.
  const int* tq_arr;
  const int* t_arr;
  int T_last;                                            // block mode: queries = keys of the LAST block (0: = T) — a row that ends inside it
  // backward with score recomputation (16-bit modes, tile-plane K / V): the pre-scaled queries Qs^T [slot][H*d][ld] of the
  // forward; q2 == nullptr = the scores are read from `scores` (kept by the forward)
  const float* q2 = nullptr; long long q2_shape_stride = 0; const int* q2_index = nullptr;
  int kv_f16 = 0;                                        // backward, one-plane mode: the K / V tile planes hold fp16 (the forward ran in math mode 3)
  // 16-bit activation maps (single-product modes): format of the register operand q (forward: Qs; backward: dO), of ctx (O),
  // of q2 and of out — 0 fp32, 1 bf16, 2 fp16; shape / evaluation strides then count 16-bit elements
  int r_fmt = 0, ctx_fmt = 0, q2_fmt = 0, out_fmt = 0;
  // score storage (block mode, two planes, tile-plane K / V): 0 = [query][key] rows of pitch Tp; 1 = TILE-MAJOR, per block
  // [key tile kt][query][32 keys] (the 128 bytes of a query's tile, fp32 scores or [hi 32 | lo 32] planes): what a wave stores
  // or loads per instruction is then one contiguous run instead of sixteen 64-byte pieces 2 KB apart
  int sc_layout = 0;
  // backward, sc_tiles == 3: k and v are the same tile planes (folded projections; bf16x3, d = 256) — every tile is fetched
  // once and committed into both LDS images (attn_bf16x3.hip KV_SAME).  Set by the C-ABI entry point alone
  int kv_same = 0;
};
extern int csn_dev_kv_same;                              // development switch (csn_dev_set): 1 = the entry point may set it
// development switch: 1 = the d = 256 bf16x3 no-planes backward launches its 64-query instance (attn_bf16x3.hip WG64) where k and v
// are the same planes; and how many launches took it since the library was loaded
extern int csn_dev_attn_wg64, csn_dev_attn_wg64_launches;
// score recomputation needs three LDS tile images per stage: one plane at every width, two planes up to d = 128
// (a two-plane d = 256 instance with its third image laid over the second — a timing build with wrong results — was measured
//  in round 4: 167 spilled registers, 7.2 -> 24.7 ms; profiles/r4r_recompute_d256_experiment.txt; removed with its switch)
constexpr bool csn_attn_recompute_fits(int planes, int dt) { return planes == 1 || dt <= 4; }
// ---- key-stationary dK / dV with recomputed scores (attn_dkv.hip; 16-bit modes, block mode, d <= 128) ----------------
struct CsnAttnDkvArgs {
  const float* q;     long long q_shape_stride;  const int* q_index;     // pre-scaled queries Qs^T [slot][H*d][ld], evaluation -> slot
  const float* dctx;  long long ctx_eval_stride;                          // dO^T [evaluation][H*d][ld]
  const float* k;  const float* v;                                        // tile planes (16-bit) of the slots' keys / values
  long long kv_shape_stride;  int kv_ld;  const int* kv_index;            // in 16-bit elements; evaluation -> key/value slot
  const float* lse;  const float* delta;                                  // [evaluation][H][n_blocks * T]
  float* dk;  float* dv;  long long dkv_slot_stride;                      // fp32 gradient maps [slot][..][ld]
  const int* dk_index;  const int* dv_index;                              // evaluation -> output slot (nullptr: the evaluation)
  int accumulate;
  const int* eval_ids;  const int* grp_off;  int n_groups;                // group g = eval_ids[grp_off[g] .. grp_off[g+1]); no offsets: one evaluation each
  int ld, H, T, Tp, n_blocks, T_last;
  float dropout_p;  unsigned long long seed;
  int kv_f16 = 0;                                                         // one-plane mode: k / v hold fp16 (forward of math mode 3)
  int q_fmt = 0, dctx_fmt = 0;                                            // 16-bit activation maps: 0 fp32, 1 bf16, 2 fp16 (q of a mode-3 forward)
  int out_fmt = 0;                                                        // 1: dk / dv leave as bf16 maps (written once: no accumulate)
  // cross-length / ragged geometry (math mode 1, n_blocks = 1; Tq > 0 selects it): Tq queries per evaluation (% 4) against T
  // keys (any number), k / v fp32 maps [evaluation][H*d][ld_kv] (kv_shape_stride in floats), dk / dv of the same pitch;
  // tq_arr / t_arr: per-evaluation counts of a ragged batch (device arrays; Tq, T are then the maxima that size grid and buffers)
  int Tq = 0, ld_kv = 0;
  const int* tq_arr = nullptr;  const int* t_arr = nullptr;
};
int csn_launch_attn_dkv_flash(const CsnAttnDkvArgs& a, int d, int mode, hipStream_t st);
constexpr bool csn_attn_dkv_flash_fits(int dt) { return dt <= 4; }         // K^T, V^T, dK^T, dV^T of 16 keys in one wave's registers

// ---- dV from the kept scores (attn_dv_scores.hip; math mode 1, block mode, d = 256) ----------------------------------
struct CsnAttnDvArgs {
  const float* dctx;  long long ctx_eval_stride;                          // dO^T [evaluation][H*d][ld]
  const float* scores;                                                    // the forward's S [evaluation][H][blk][T][Tp] (row- or tile-major), untouched
  const float* lse;                                                       // [evaluation][H][n_blocks * T]
  float* dv;  long long dkv_slot_stride;  const int* dv_index;            // fp32 gradient maps [slot][..][ld], evaluation -> slot
  const int* eval_ids;  const int* grp_off;  int n_groups;                // group g = eval_ids[grp_off[g] .. grp_off[g+1]); no offsets: one evaluation each
  int ld, H, T, Tp, n_blocks, T_last;
  float dropout_p;  unsigned long long seed;
  int sc_layout = 0;                                                      // 1: tile-major scores (CsnAttnArgs::sc_layout), Tp >= round-up-32(T)
};
int csn_launch_attn_dv_scores(const CsnAttnDvArgs& a, int d, int mode, hipStream_t st);
constexpr bool csn_attn_dv_scores_fits(int mode, int d) { return mode == 1 && d == 256; }   // the instance that is built

int csn_launch_attn_fwd_f32(const CsnAttnArgs& a, int d, hipStream_t st);
int csn_launch_attn_bwd_f32(const CsnAttnArgs& a, int d, hipStream_t st);
int csn_launch_attn_fwd_bf16x3(const CsnAttnArgs& a, int d, int mode, hipStream_t st);     // attn_bf16x3.hip; mode 1..3 (2, 3: tile-plane K/V only)
int csn_launch_attn_bwd_bf16x3(const CsnAttnArgs& a, int d, int mode, hipStream_t st);     // mode 1, 2

// ---- output projection + residual + LayerNorm (outproj_ln.hip) --------------------------------
struct CsnOutProjArgs {
  const float* ctx;   long long ctx_eval_stride;         // Ctx^T[e][D][ld]
  const float* wfc;                                      // [C][D] row-major (csa_models.py:52)
  const float* xres;  long long xres_shape_stride; const int* res_index;   // residual x[shape][C][ld] (:99,:116)
  float* xhat;        long long xhat_eval_stride;        // normalised output [e][C][ld]
  float* rstd;                                           // [e][n_points]
  int E, C, D, ld, n_points;
  float eps;
  float dropout_p;                                       // dropout on the fc output (csa_models.py:115); 0 = off
  unsigned long long seed;
  // optional: xhat_sum[e][c] = sum over points of xhat (the pooled descriptor of csa_models.py:211-212 before the affine).
  // The 256 x 256-tile kernel forms per-tile partial sums in its epilogue (sum_ws [e][ceil(n_points/256)][C], reduced by a
  // small second kernel in fp64); the other kernels are followed by the streaming row-sum pass.
  float* xhat_sum; float* sum_ws; long long sum_ws_floats;
  // 16-bit activation maps (math modes 2 / 3): ctx is a 16-bit map of the mode's type, xhat leaves as fp16; strides in elements
  int act16 = 0;
};
int csn_launch_partial_sums_f32(const float* ws, float* out, long long rows_outer, int tiles, int C, hipStream_t st);
int csn_launch_outproj_ln_fwd_f32(const CsnOutProjArgs& a, int mode, hipStream_t st);   // mode 0: fp32, 1..3: 16-bit matrix-core contraction
int csn_launch_outproj_ln_big(const CsnOutProjArgs& a, int mode, hipStream_t st);       // gemm_bf16x3.hip: C = 256, 256 x 256 tiles

// masked cross-entropy on class-major logits (loss.hip; csa_training.py:94-108)
struct CsnMaskedCeArgs {
  const float* logits;  long long shape_stride;  int ld;          // [shape][class][ld]
  const long long* labels;  long long label_shape_stride;         // [shape][n_points] int64
  int n_shapes, n_classes, n_points, mask;                        // counted: mask < label < n_classes
  float* lse;                                                     // [shape][n_points]  (metrics form: may be null)
  int* pred;  int* counts;                                        // metrics form (counts != null): [shape][n_points] arg-max (may be
                                                                  // null), [shape][class][3] inter / gt / pr over label > mask
  double* partials;                                               // forward: 3 per block (csn_masked_ce_blocks)
  float* stats;                                                   // [3]: mean loss, accuracy, counted points
  const float* grad_out;  float* dlogits;  long long dshape_stride;  int dld;      // backward
};
long long csn_masked_ce_blocks(int n_shapes, int n_points);
int csn_launch_masked_ce_fwd(const CsnMaskedCeArgs& a, hipStream_t st);
int csn_launch_masked_ce_bwd(const CsnMaskedCeArgs& a, hipStream_t st);

struct CsnLnBwdArgs {
  const float* dxhat; const float* xhat; const float* rstd;   // [e][C][ld], [e][C][ld], [e][n_points]
  const float* dxhat_rows;                                     // optional [e][C]: added to every point of row (e, c)
  int n_dense;                                                 // evaluations e >= n_dense have no dense dxhat (only the row term)
  // dense part of evaluation e < n_dense = dxhat_scale[e][c] * dxhat[e / dxhat_group][c][n]  (scale null: 1; group 1: map e).
  // With group = K+1 and scale = comp * gamma the maps are the gradient of the mixed features themselves: the per-evaluation
  // gradient maps of the mix are never written
  const float* dxhat_scale; int dxhat_group;
  float* dz;                                                   // [e][C][ld]  gradient w.r.t. the fc output (dropout mask applied)
  float* dz_res;                                               // optional: gradient w.r.t. the residual input (no mask)
  long long eval_stride;
  int E, C, ld, n_points;
  float dropout_p;
  unsigned long long seed;
  int act16 = 0;                                               // xhat is an fp16 map, dz leaves as a bf16 map (dxhat, dz_res stay fp32)
  int e_base = 0;                                              // the launch covers evaluations e_base .. e_base + E - 1 of the maps
};
int csn_launch_ln_bwd_f32(const CsnLnBwdArgs& a, hipStream_t st);
// LayerNorm backward fused into the dCtx stream (wx_lnb.hip; bf16x3, d_model = d_inner = 256, fp32 maps)
struct CsnWxLnbArgs {
  const float* w;                                              // W_fc^T [d_inner][d_model] row-major
  const float* xhat; const float* rstd; long long eval_stride; int ld;
  const float* dxhat; int dxhat_group; int n_dense; const float* dxhat_scale; const float* dxhat_rows;     // as CsnLnBwdArgs
  float* dz; float* dz_res;                                    // [e][256][ld]; dz_res optional
  float* dctx; long long dctx_eval_stride;                     // [e][256][ld]
  int n_items, n_points, e_base;                               // evaluations e_base .. e_base + n_items - 1
  float dropout_p; unsigned long long seed;
  // optional, e_base = 0 and every evaluation of the launch dense: the mix backward's reductions from the same pass —
  // rowdot[e][256] = sum_n dxhat[e / group][c][n] xhat[e][c][n], rowsum[e / group][256] = sum_n dxhat[e / group][c][n] (raw
  // dxhat, before scale and rows); red_ws: csn_wx_lnb_red_floats(n_items, n_points) floats, red_slots = csn_wx_ln_sum_slots(..)
  float* red_ws; int red_slots; float* rowdot; float* rowsum;
};
long long csn_wx_lnb_red_floats(int n_items, int n_points);
bool csn_wx_lnb_takes(const CsnLnBwdArgs& a, int d_inner);
int csn_launch_wx_lnb(const CsnWxLnbArgs& a, hipStream_t st);

// delta[e][h][n] = sum_{c in head h} a[e][c][n] * b[e][c][n]
int csn_launch_rowdot_f32(const float* a, const float* b, float* out, const int* eval_ids, int E, int H, int d, int ld,
                          int n_points, long long eval_stride, int a_split, long long a_plane_stride, hipStream_t st);

// ---- pooled descriptors / cross-shape mix (combine.hip) ---------------------------------------------
// x16 != 0: the normalised maps (x / xhat / xhat0) are fp16 (16-bit activation maps)
int csn_launch_rowsum_f32(const float* x, float* out, long long rows, int n, long long ld, hipStream_t st, int x16 = 0);
int csn_launch_mix_fwd_f32(const float* xhat, const float* comp, const float* gamma, const float* beta, float* feats, int B,
                           int K1, int C, int NP, const float* xhat0, hipStream_t st, int x16 = 0);
int csn_launch_mix_bwd_f32(const float* dfeats, const float* xhat, const float* comp, const float* gamma, float* dxhat,
                           float* rowdot, float* rowsum, int B, int K1, int C, int NP, const float* xhat0, float* dxhat0,
                           hipStream_t st, int x16 = 0);
int csn_launch_retrieval_f32(const float* f1, const float* f2, float* out, int s1, int n1, int s2, int n2, int C,
                             float* ws, hipStream_t st);

// ---- ragged MinkowskiNet head (minkowski_csn.hip) and ragged retrieval (retrieval.hip) --------------
int csn_ragged_mix_tiles(int max_points);
int csn_launch_ragged_pool_f32(const float* xhat, long long eval_stride, int ld, const int* counts, int E, int C, const float* gamma,
                               const float* beta, float* pooled, float* mean, hipStream_t st);
int csn_launch_ragged_pool_bwd_f32(const float* dpooled, const float* gamma, const int* counts, int E, int C, float* dxhat,
                                   long long eval_stride, int ld, int accumulate, hipStream_t st);
int csn_launch_ragged_mix_fwd_f32(const float* xhat, long long eval_stride, int ld, int cross_first, const int* offsets, int B,
                                  int K1, int C, int max_points, const float* comp, const float* gamma, const float* beta, float* out,
                                  long long ld_out, hipStream_t st);
int csn_launch_ragged_mix_bwd_f32(const float* dout, long long ld_dout, const float* xhat, long long eval_stride, int ld,
                                  int cross_first, const int* offsets, int B, int K1, int C, const float* comp, const float* gamma,
                                  float* dxhat, double* rowdot, double* rowsum, double* ws, hipStream_t st);
int csn_launch_ragged_retrieval_f32(const float* f1, const int* off1, int s1, long long N1, const float* f2, const int* off2, int s2,
                                    long long N2, int max_n1, int C, float* out, float* ws, hipStream_t st);
int csn_launch_ragged_mean_f32(const float* part, const int* off1, float* out, int pairs, int s2, int tiles, hipStream_t st);
// the same arithmetic for a device list of (i, j) pairs: out[p] (retrieval.hip)
int csn_launch_ragged_retrieval_pairs_f32(const float* f1, const int* off1, int s1, long long N1, const float* f2, const int* off2,
                                          int s2, long long N2, int max_n1, int C, const int* pairs, long long n_pairs, float* out,
                                          float* ws, hipStream_t st);
// fp16 screen of the ragged retrieval measure (retrieval_screen.hip): the sweep keeps 128 query rows and two 64-row candidate
// tiles of Cp + 8 halves in LDS, 512 (Cp + 8) bytes of the CU's 160 KB
#define CSN_SCREEN_MAX_CP 288
int csn_screen_padded_channels(int C);
int csn_launch_ragged_retrieval_screen_f16(const float* f1, const int* off1, int s1, long long N1, const float* f2, const int* off2,
                                           int s2, long long N2, int max_n1, int C, float* out, float* ws, hipStream_t st);

// ---- loss, predictions and IoU counts of the MinkowskiNet head on point-major ragged rows (minkowski_seg.hip) ----
struct CsnRaggedSegArgs {
  const float* logits;  int n_rows;  int ld;                      // [row][ld], n_classes <= ld
  const long long* labels;                                        // [row] int64
  const int* offsets;  int n_segments;                            // device copy, [n_segments + 1]
  int n_classes, ignore_label;
  float* lse;  float* nll;  int* pred;                            // [row]; nll = the row's loss (0 for an uncounted row)
  double* stats;                                                  // [4]: mean loss, counted, correct, bad rows
  int* counts;                                                    // [segment][class][3]: inter, gt, pr
  double* partials;                                               // forward: 4 per work-group (csn_ragged_seg_blocks)
  const float* grad_out;  float* dlogits;  int dld;               // backward
  int pitch = 0, vec = 0;                                         // set by the launcher
};
long long csn_ragged_seg_blocks(int n_rows);
int csn_launch_ragged_seg_fwd(const CsnRaggedSegArgs& a, hipStream_t st);
int csn_launch_ragged_seg_bwd(const CsnRaggedSegArgs& a, hipStream_t st);

// ---- compatibility head (compat.hip): normalize(W_q y_0 + b), normalize(W_k y_k + b), dot, softmax over the K+1 keys ----
int csn_launch_compat_fwd(const float* pooled, const float* wq_t, const float* bq, const float* wk_t, const float* bk, float* comp,
                          double* save_u, double* save_n, int B, int K1, int C, int reference_layout, hipStream_t st);
int csn_launch_compat_bwd(const float* dcomp, const float* comp, const double* save_u, const double* save_n, const float* pooled,
                          const float* wq, const float* wk, double* d_raw, double* dx, float* dpooled, float* dwq, float* dbq,
                          float* dwk, float* dbk, int B, int K1, int C, int reference_layout, hipStream_t st);

// ---- fc_layer of the MinkowskiNet head on point-major rows: 1x1 convolution + BatchNorm + ReLU (rows_fc.hip) ----
struct CsnRowsFcArgs {
  const float* x;  int ld_x;                                      // [n_rows][ld_x], c_in <= ld_x
  const float* w;  const float* bias;                             // [c_out][c_in] row-major; bias optional
  const float* gamma;  const float* beta;
  float* running_mean;  float* running_var;  float eps, momentum;
  int training, n_rows, c_in, c_out;
  float* y;  int ld_y;                                            // forward: written; backward: read (the ReLU mask is y > 0)
  float* z;  int ld_z;                                            // training: x w^T + bias, kept for the backward
  float* mean;  float* invstd;                                    // training: the batch's; eval backward: running mean / variance
  const float* dy;  int ld_dy;
  float* dx;  int ld_dx;  float* dw;  float* dbias;  float* dgamma;  float* dbeta;
  void* ws;
};
long long csn_rows_fc_ws_bytes(long long n_rows, int c_in, int c_out, int training, int backward);
int csn_launch_rows_fc_fwd(const CsnRowsFcArgs& a, int mode, hipStream_t st);
int csn_launch_rows_fc_bwd(const CsnRowsFcArgs& a, int mode, hipStream_t st);
// fp64 column sums of [n_rows][C] rows in a fixed order (the bias gradients): part[chunk][C] of 64-row chunks (four waves each
// taking every fourth row, added in wave order), then the chunks in 32 segments added in segment order; C % 32 == 0
int csn_launch_rows_colsum(const float* x, int ldx, long long n_rows, int C, double* part, hipStream_t st);
int csn_launch_rows_colsum_merge(const double* part, int n_chunks, int C, float* out, hipStream_t st);

// ---- sparse 3D convolution on voxel rows over a kernel map (sparse_conv.hip) ----
struct CsnSparseConvArgs {
  const float* x;  int ld_x;  int n_in;                           // [n_in][ld_x], c_in <= ld_x
  const int* fwd_table;  const int* bwd_table;                    // [kv][n_out] input row or -1; [kv][n_in] output row or -1 (NULL: fwd reversed)
  int n_out, kv, c_in, c_out;
  const float* w;  const float* bias;                             // [kv][c_in][c_out]; bias optional
  float* y;  int ld_y;                                            // forward: [n_out][ld_y]
  const float* dy;  int ld_dy;
  float* dx;  int ld_dx;  float* dw;  float* dbias;               // each skipped when NULL
  void* ws;
  int w_rows;                                                     // forward only: rows of every W[k] (0: c_in); > c_in: w is a row slice
};
long long csn_sparse_conv_ws_bytes(long long n_in, long long n_out, int kv, int c_in, int c_out, int backward);
int csn_launch_sparse_conv_fwd(const CsnSparseConvArgs& a, int mode, hipStream_t st);
int csn_launch_sparse_conv_bwd(const CsnSparseConvArgs& a, int mode, hipStream_t st);
// forward with the BatchNorm statistics epilogue (no bias): a.y = z, a.ws = csn_sparse_conv_stats_ws_bytes(n_out, c_out) bytes.
// group_rows (NULL, 0: the whole map is one batch): as for csn_launch_rows_bn_act_fwd below, mean / invstd [n_groups][c_out]
long long csn_sparse_conv_stats_ws_bytes(long long n_out, int c_out);
int csn_launch_sparse_conv_stats_fwd(const CsnSparseConvArgs& a, const int* group_rows, int n_groups, float* mean, float* invstd,
                                     float* running_mean, float* running_var, float eps, float momentum, int mode, hipStream_t st);
// forward with the inference epilogue (no bias): a.y = act(z s + t + r), s = gamma / sqrt(running_var + eps), t = beta -
// running_mean s; r optional, may be a.y itself with ld_r == a.ld_y.  One launch, no workspace
struct CsnSconvBnArgs {
  const float* gamma;  const float* beta;  const float* running_mean;  const float* running_var;  float eps;
  const float* r;  int ld_r;  int relu;
};
int csn_launch_sparse_conv_bn_act_fwd(const CsnSparseConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);
// (27) the same over a concatenation that is never formed (sparse_conv_cat.hip): x[m] / ld_x[m] / c_in[m] the parts, a.c_in the sum of
// their widths, a.w the one kernel [kv][a.c_in][c_out]; a chain of one launch per part, the last with the statistics epilogue
int csn_launch_sparse_conv_cat_stats_fwd(const CsnSparseConvArgs& a, const float* const* x, const int* ld_x, const int* c_in, int n_parts,
                                         float* mean, float* invstd, float* running_mean, float* running_var, float eps, float momentum,
                                         int mode, hipStream_t st);
extern int csn_dev_sconv_nb;                                      // development switch (csn_dev_set): 0 = the launch rule
// the 32-column blocks a wave owns in a gather-GEMM of J columns over M rows: sparse_conv.hip's launch rule, csn_dev_sconv_nb included
int csn_sconv_column_blocks(int J, long long M);
// the same forward with the inference epilogue on 16-bit maps (sparse_conv_maps16.hip; math modes 2 / 3, single product): x, r and
// y are each fp32 rows (flag 0) or rows of the mode's 16-bit type (flag 1), pitches in elements of the map's own type; the vectors,
// eps and relu come from CsnSconvBnArgs (its r / ld_r are not read)
struct CsnSparseConvM16Args {
  const void* x;  int x16;  int ld_x;  int n_in;
  const int* table;  int n_out, kv, c_in, c_out;
  const float* w;
  const void* r;  int r16;  int ld_r;                             // optional; may be y itself with the same type and pitch
  void* y;  int y16;  int ld_y;
};
int csn_launch_sparse_conv_bn_act_fwd_m16(const CsnSparseConvM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);

// ---- kernel-2 stride-2 convolution and its transposed form over an octant map (octant_conv.hip) ----
struct CsnOctantConvArgs {
  const float* x;  int ld_x;                                      // down: [n_fine][ld_x]; up: [n_coarse][ld_x]; c_in <= ld_x
  int n_fine, n_coarse, c_in, c_out;
  const int* children;                                            // [8][n_coarse] fine row or -1
  const int* parent;  const int* order;  const int* seg;          // [n_fine], [n_fine], [9]
  const float* w;  const float* bias;                             // [8][c_in][c_out]; bias optional
  float* y;  int ld_y;                                            // forward: down [n_coarse][ld_y], up [n_fine][ld_y]
  const float* dy;  int ld_dy;
  float* dx;  int ld_dx;  float* dw;  float* dbias;               // each skipped when NULL
  void* ws;
};
long long csn_octant_conv_ws_bytes(long long n_fine, long long n_coarse, int c_in, int c_out, int up, int backward);
int csn_launch_octant_down_fwd(const CsnOctantConvArgs& a, int mode, hipStream_t st);
int csn_launch_octant_down_bwd(const CsnOctantConvArgs& a, int mode, hipStream_t st);
int csn_launch_octant_up_fwd(const CsnOctantConvArgs& a, int mode, hipStream_t st);
int csn_launch_octant_up_bwd(const CsnOctantConvArgs& a, int mode, hipStream_t st);
// the two forwards with the inference epilogue of CsnSconvBnArgs (no bias): a.y = act(z s + t + r), one launch, no workspace
int csn_launch_octant_down_bn_act_fwd(const CsnOctantConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);
int csn_launch_octant_up_bn_act_fwd(const CsnOctantConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);
// the 32-column blocks a wave owns in a one-weight product of J columns over M rows: octant_conv.hip's launch rule
int csn_octant_column_blocks(int J, long long M);
// the two forwards with the BatchNorm statistics epilogue (include/csn_hip.h section 26, octant_conv_stats.hip): a.y = z, no bias,
// a.ws = csn_octant_stats_ws_bytes bytes; down is csn_launch_sparse_conv_stats_fwd over children as a table of 8 offsets
long long csn_octant_stats_ws_bytes(long long n_fine, long long n_coarse, int c_out, int up);
int csn_launch_octant_down_stats_fwd(const CsnOctantConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                     float eps, float momentum, int mode, hipStream_t st);
int csn_launch_octant_up_stats_fwd(const CsnOctantConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                   float eps, float momentum, int mode, hipStream_t st);
// the same two forwards as ONE 16-bit product (math modes 2 / 3) on maps that are each fp32 or 16-bit rows
// (octant_conv_maps16.hip): down is csn_launch_sparse_conv_bn_act_fwd_m16 over children as a table of 8 offsets, up kernels of
// their own; the vectors, eps and relu come from CsnSconvBnArgs (its r / ld_r are not read)
struct CsnOctantM16Args {
  const void* x;  int x16;  int ld_x;
  int n_fine, n_coarse, c_in, c_out;
  const int* children;                                            // down
  const int* parent;  const int* order;  const int* seg;          // up
  const float* w;
  const void* r;  int r16;  int ld_r;                             // optional; may be y itself with the same type and pitch
  void* y;  int y16;  int ld_y;
};
int csn_launch_octant_down_bn_act_fwd_m16(const CsnOctantM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);
int csn_launch_octant_up_bn_act_fwd_m16(const CsnOctantM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st);

// ---- BatchNorm apply + branch sum + residual + ReLU on point-major rows, forward and backward (rows_bn_act.hip) ----
struct CsnRowsBnActArgs {
  // the terms (include/csn_hip.h section 15: CsnBnTerms, copied by the C ABI)
  const float* z[3];  int ld_z[3];
  const float* mean[3];  const float* scale[3];  const float* gamma[3];  const float* beta[3];
  float* dz[3];  int ld_dz[3];  float* dgamma[3];  float* dbeta[3];
  int n_terms;
  int n_rows, C, training, relu;  float eps;
  const float* r;  int ld_r;                                      // residual, optional
  float* y;  int ld_y;                                            // forward: written; backward: read (the ReLU mask is y > 0)
  const float* dy;  int ld_dy;
  float* dr;  int ld_dr;
  void* ws;
};
// group_rows (device, n_groups + 1 entries; NULL, 0: the whole map is one BatchNorm batch): group g is the rows [group_rows[g],
// group_rows[g + 1]) and a batch of its own, mean / scale of the terms are [n_groups][C]; training mode only.
// the Chan merge of [tile][2][C] (mean, M2) partials of 32-row tiles (the statistics epilogue of sparse_conv.hip): mean, invstd,
// running statistics (either may be NULL); z, ld_z: the map itself, read only where a group boundary cuts a tile
int csn_launch_bn_stats_merge(const float* part, int n_tiles, int n_rows, int C, float eps, float momentum, const float* z, int ld_z,
                              const int* group_rows, int n_groups, float* mean, float* invstd, float* running_mean, float* running_var,
                              hipStream_t st);
long long csn_rows_bn_act_ws_bytes(long long n_rows, int C, int n_terms, int n_groups);      // n_groups 1: the whole map
int csn_launch_rows_bn_act_fwd(const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, hipStream_t st);
// the backward is pass 1 (dr, the chunks' sums), the sums, pass 2 (dz); `pass` launches row pass 1 or 2 on the workspace's parts and
// coefficients (NULL: the fp32 kernels of rows_bn_act.hip)
typedef int (*CsnBnActPass)(int pass, const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, double* part, const float* coef,
                            int n_parts, hipStream_t st);
int csn_launch_rows_bn_act_bwd(const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, hipStream_t st, CsnBnActPass pass = nullptr);

// ---- the HRNet backbone's training step on bf16 activation maps (train_maps16.hip; math mode 2, single product) ----
// The launches above with ONE map read or written as bf16 rows (pitch in elements, a multiple of 8) where the fp32 form's first use of
// it is a rounding to bf16: a.x of the statistics forward and of the weight gradient (cast to const float* in the argument struct),
// y and r of the BatchNorm row kernels.  Every sum is the fp32 form's, in its order.
int csn_launch_sparse_conv_stats_fwd_x16(const CsnSparseConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                         float eps, float momentum, hipStream_t st);
int csn_launch_sparse_conv_wgrad_x16(const CsnSparseConvArgs& a, hipStream_t st);           // a.dw alone, from a.x (bf16), a.dy, a.ws
int csn_launch_rows_bn_act_fwd16(const CsnRowsBnActArgs& a, int r16, int y16, hipStream_t st);
int csn_launch_rows_bn_act_bwd16(const CsnRowsBnActArgs& a, hipStream_t st);                // a.y: bf16 rows
// the weight gradient's launch plan (sparse_conv.hip): the 32-row blocks of c_in per work-group, the split-K chunks and where the
// chunks' slabs lie in the backward's workspace
void csn_sconv_wgrad_plan(long long n_out, int kv, int c_in, int c_out, int* ta, int* splits, int* chunk, long long* slabs_offset);

// ---- point fields: voxel means, trilinear interpolation onto points and its adjoint (point_field.hip) ----
struct CsnPointFieldArgs {
  const float* coords;                                            // [n_points][4] = [b, x, y, z] in voxel units, 16-byte aligned
  const int* home;                                                // [n_points] the voxel row of floor(xyz)
  const int* vox_ptr;  const int* vox_pts;                        // the points of every voxel as a CSR: [n_voxels + 1], [n_points]
  const int* table;                                               // [27][n_voxels]: the kernel-3 stride-1 map, -1 = no voxel
  int n_points, n_voxels, C;
  const float* z;  long long ld_z;                                // forward: the voxel map, read
  float* y;  long long ld_y;                                      // forward: the point map, written
  const float* dy;  long long ld_dy;                              // backward: read (voxel_mean: the point features)
  float* dz;  long long ld_dz;                                    // backward: written (voxel_mean: the means)
};
int csn_launch_voxel_mean(const CsnPointFieldArgs& a, hipStream_t st);
int csn_launch_point_interp_fwd(const CsnPointFieldArgs& a, hipStream_t st);
int csn_launch_point_interp_bwd(const CsnPointFieldArgs& a, hipStream_t st);

// ---- kernel maps: packed coordinate keys, the coarser level's keys, the offset tables by binary search (kernel_map.hip) ----
struct CsnKernelMapArgs {
  const long long* set_keys;                                      // [n_set] ascending packed keys of the searched set
  const int* set_rows;                                            // [n_set] the row of every sorted key, or NULL: the position itself
  const long long* query_keys;                                    // [n_query] packed keys of the rows the table is indexed by
  int n_set, n_query, kernel_size, step;                          // step: sign * offset step, non-zero
  int* table;                                                     // [kernel_size^3][n_query], written
  int* status;                                                    // one word, or-ed into (8: the set is not strictly ascending)
};
int csn_launch_coord_keys(const long long* coords, int n, int tensor_stride, long long* keys, int* status, hipStream_t st);
int csn_launch_coord_down(const long long* keys, int n, int out_tensor_stride, long long* down_keys, hipStream_t st);
int csn_launch_kernel_map(const CsnKernelMapArgs& a, hipStream_t st);

// ---- octant maps: parent, octant and children of a fine set by one search per row; the rows sorted by octant (octant_map.hip) ----
struct CsnOctantMapArgs {
  const long long* fine_keys;                                     // [n_fine] packed keys of the fine rows, in row order
  const long long* fine_sorted;                                   // [n_fine] the same keys ascending, or NULL: their neighbours are not checked
  const long long* coarse_keys;                                   // [n_coarse] ascending packed keys of the coarse set
  const int* coarse_rows;                                         // [n_coarse] the row of every sorted key, or NULL: the position itself
  int n_fine, n_coarse, tensor_stride;                            // tensor_stride: the fine set's
  int* parent;  int* octant;                                      // [n_fine], written
  int* children;                                                  // [8][n_coarse], filled with -1 and written
  int* status;                                                    // one word, or-ed into (8: a set is not strictly ascending, 16: no parent)
};
constexpr int CSN_OCTANT_ORDER_TILE = 256;                        // rows per work-group of the count and scatter launches
constexpr int CSN_OCTANT_ORDER_SCAN = 256;                        // tiles per pass of the scan's one work-group
int csn_launch_octant_partition(const CsnOctantMapArgs& a, hipStream_t st);
long long csn_octant_order_tiles(int n);
int csn_launch_octant_order(const int* octant, int n, int* order, int* seg, int* counts, int* status, hipStream_t st);  // counts: [8][tiles]

// ---- resident point collections: normalise, bound, augment + collate + key, and a PointField's index arrays (points.hip) ----
constexpr int CSN_POINTS_NPARAM = 9;                              // per item: cos, sin, shift_z[3], jitter[3], scale
struct CsnPointsArgs {
  const float* points;                                            // [n_total][3] the collection, flat
  const int* labels;                                              // [n_total] or NULL
  const long long* offsets;                                       // [n_shapes + 1] the rows of every shape
  int n_shapes;  long long n_total;
  float* out;  int method;                                        // normalize: [n_total][3] written (may be points); 0 sphere, 1 box
  const long long* idx;                                           // [n_items] the shape of every batch item
  const long long* out_offsets;                                   // [n_items] the first output row of every item
  const double* params;                                           // [n_items][CSN_POINTS_NPARAM]
  double* bounds;                                                 // [n_items][6] min xyz, max xyz of the rotated points (bounds: written)
  int n_items, max_points;                                        // max_points: the longest shape among the items
  double sigma, clip, voxel_size;
  float* coords;  float* feats;  long long* labels_out;  long long* keys;  long long n_out;      // batch: written, n_out rows
  int* status;                                                    // one word, or-ed into
};
int csn_launch_points_normalize(const CsnPointsArgs& a, hipStream_t st);
int csn_launch_points_bounds(const CsnPointsArgs& a, hipStream_t st);
int csn_launch_points_batch(const CsnPointsArgs& a, hipStream_t st);
int csn_launch_field_index(const long long* skeys, const long long* order, const long long* vid, int n_points, int n_voxels, int* home,
                           int* vox_ptr, int* vox_pts, long long* uniq_keys, int* status, hipStream_t st);
