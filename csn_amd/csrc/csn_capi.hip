// extern "C" surface of libcsn_hip.so (declared in include/csn_hip.h).  Argument checking and the
// decomposition of each domain-level call into kernel launches live here; no allocation, no sync.
#include "../../include/csn_hip.h"
#include "csn_kernels.h"
#include <cmath>

namespace {

// 0: exact fp32 matrix cores; 1: bf16x3 (three bf16 products per fp32 product); 2: bf16; 3: fp16 (one product)
int g_math_mode = CSN_MATH_BF16X3;          // process default (csn_set_math_mode)
thread_local int t_math_mode = -1;          // per-thread override (csn_set_thread_math_mode); -1 = none

inline int mode() { return t_math_mode >= 0 ? t_math_mode : g_math_mode; }
// 16-bit activation maps between the entry points (csn_set_thread_act16): 0 off, 1 = the forward's maps are bf16 (math mode 2),
// 2 = they are fp16 (math mode 3 forward; its backward runs in mode 2 and converts them while staging)
// + 4: the gradient maps dQ / dK / dV (and what reads them: the projection weight gradients, dx) are bf16 maps too
thread_local int t_act16 = 0;
inline int act16() { return t_act16 & 3; }
inline bool grad16() { return (t_act16 & 4) != 0; }
// forward entry points: the flag has to name the type of the mode that runs; backward: mode 2 takes either
inline bool act16_fwd_ok() { return act16() == 0 || (act16() == 1 && mode() == 2) || (act16() == 2 && mode() == 3); }
inline bool act16_bwd_ok() { return act16() == 0 || mode() == 2; }
// single-product row products of sections 13 / 14 / 15a (csn_set_thread_rows16): 0 = modes 2 / 3 run as mode 1 there, 1 = they
// run the bf16 / fp16 instances
thread_local int t_rows16 = 0;
inline int rows_mode() { return mode() >= 2 && !t_rows16 ? 1 : mode(); }
// score storage of the block-attention entry points (csn_set_thread_score_layout): 0 = [query][key] rows, 1 = tile-major
thread_local int t_score_layout = 0;
inline int planes_of(int m) { return m == 1 ? 2 : 1; }          // tile-plane / split-tensor planes of a 16-bit mode

// the cross-length entry points (fp32 K / V maps) have no single-product kernels: in modes 2 / 3 they run as mode 1
struct ModeGuard {
  int saved;
  explicit ModeGuard(int m) : saved(t_math_mode) { t_math_mode = m; }
  ~ModeGuard() { t_math_mode = saved; }
};

int launch_gemm(const CsnGemmArgs& a, int b_is_nk, int batch, hipStream_t st) {
  if (mode() != 0) {
    if (a.M <= 0 || a.N <= 0 || batch <= 0) return 0;
    if ((a.A.ld & 3) || (a.B.ld & 3) || (a.K & 3) || (a.k_chunk & 3)) return CSN_E_ALIGN;
    if (a.N & 3) return CSN_E_ALIGN;               // (k-contiguous B too: the 256 x 256 epilogues write 16-byte chunks of C)
    return csn_launch_gemm_bf16x3(a, b_is_nk, batch, mode(), st);
  }
  return csn_launch_gemm_f32(a, b_is_nk, batch, st);
}

inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// K = 256 weight products of the bf16x3 mode on the weight-stationary streaming kernel (wx_stream.hip)
int launch_wx(const float* w, const float* x, long long x_stride, int ldx, void* out, long long out_stride, int ldo, int rows,
              int n_items, int n_points, int div_rows, float div_val, int out_mode, int tb, hipStream_t st) {
  CsnWxArgs a;
  a.w = w; a.x = x; a.x_item_stride = x_stride; a.ldx = ldx;
  a.out = out; a.out_item_stride = out_stride; a.ldo = ldo;
  a.n_items = n_items; a.n_points = n_points; a.n_sets = rows / 256;
  a.div_rows = div_rows; a.div_val = div_val; a.div_rcp = 1.f / div_val;
  int ex = 0;
  a.div_exact = (std::frexp(div_val, &ex) == 0.5f && div_val > 0.f) ? 1 : 0;     // a power of two: v * (1 / t) == v / t bit for bit
  a.tb = tb;
  return csn_launch_wx(a, out_mode, st);
}

// Block mode, n_blocks * block > ld: the row of ld points ends inside the last block, which then holds
// ld - (n_blocks - 1) * block points (a multiple of 4).  Returns that count, 0 for full blocks, or a negative status.
inline int last_block_points(int block, int n_blocks, int ld, int block_q) {
  if (block_q != 0) return 0;                                  // cross-length entries: key and query counts are explicit
  if ((long long)n_blocks * block <= ld) return 0;
  if ((long long)(n_blocks - 1) * block >= ld) return CSN_E_ARG;
  const int t = ld - (n_blocks - 1) * block;
  return (t & 3) ? CSN_E_ALIGN : t;
}
inline bool dim_ok(int d) { return d == 32 || d == 64 || d == 96 || d == 128 || d == 256; }

CsnOperand operand(const float* p, long long s0, long long s1, long long s2, const int* idx2, int ld) {
  CsnOperand o;
  o.ptr = const_cast<float*>(p);
  o.s0 = s0; o.s1 = s1; o.s2 = s2; o.idx2 = idx2; o.ld = ld;
  o.planes = 0; o.plane_stride = 0;
  return o;
}

// points contracted per work-group of a split weight gradient
int wgrad_chunk(int n_maps, int n_points) {
  // ~512 equal slabs: every map is cut into the same number of equal chunks (unequal tails leave CUs idle at the end)
  long long total = (long long)n_maps * n_points;
  long long want = (total + 511) / 512;
  if (want < 256) want = 256;
  long long n_chunks = (n_points + want - 1) / want;
  if (n_chunks < 1) n_chunks = 1;
  long long c = (n_points + n_chunks - 1) / n_chunks;
  c = ((c + 3) / 4) * 4;
  return (int)c;
}

// dw[rows][cols] (+)= scale * sum_{z2, n} a[z2][rows][n] * b[z2][cols][n]      (a_fmt / b_fmt: CSN_FMT_* of the two maps)
int wgrad(const float* a, long long a_stride, int lda, const float* b, long long b_stride, int ldb, float* dw, int rows,
          int cols, int n_maps, int n_points, float scale, int accumulate, float* ws, long long ws_floats,
          hipStream_t st, int a_fmt = 0, int b_fmt = 0) {
  const int chunk = wgrad_chunk(n_maps, n_points);
  const int n_chunks = (n_points + chunk - 1) / chunk;
  const long long slabs = (long long)n_maps * n_chunks;
  if (ws_floats < slabs * rows * cols) return CSN_E_WORKSPACE;
  CsnGemmArgs g;
  g.A = operand(a, chunk, 0, a_stride, nullptr, lda);
  g.B = operand(b, chunk, 0, b_stride, nullptr, ldb);
  g.A.fmt = a_fmt; g.B.fmt = b_fmt;
  g.C = operand(ws, (long long)rows * cols, 0, (long long)n_chunks * rows * cols, nullptr, cols);
  g.M = rows; g.N = cols; g.K = n_points;
  g.n0 = n_chunks; g.n1 = 1; g.k_chunk = chunk;
  g.alpha = 1.f; g.div_rows = 0; g.div_val = 1.f; g.accumulate = 0; g.eval_ids = nullptr;
  int rc = launch_gemm(g, /*b_is_nk=*/1, (int)slabs, st);
  if (rc) return rc;
  return csn_launch_slab_reduce(ws, dw, (int)slabs, (long long)rows * cols, scale, accumulate, st);
}

}  // namespace

extern "C" {

int csn_version(void) { return CSN_ABI_VERSION; }

int csn_dev_get(int key) {
  switch (key) {
    case CSN_DEV_BIG_TILES: return csn_gemm_big_tiles;
    case CSN_DEV_WIDE_GEMM: return csn_gemm_wide;
    case CSN_DEV_WIDE_FORMS: return csn_gemm_wide_set;
    case CSN_DEV_WX: return csn_dev_wx;
    case CSN_DEV_LNB_GROUP: return csn_dev_lnb_group;
    case CSN_DEV_SCONV_NB: return csn_dev_sconv_nb;
    case CSN_DEV_KV_SAME: return csn_dev_kv_same;
    case CSN_DEV_ATTN_WG64: return csn_dev_attn_wg64;
    case CSN_DEV_ATTN_WG64_LAUNCHES: return csn_dev_attn_wg64_launches;
    default: return CSN_E_ARG;
  }
}
int csn_dev_set(int key, int value) {
  const int prev = csn_dev_get(key);
  switch (key) {
    case CSN_DEV_BIG_TILES: csn_gemm_big_tiles = value; break;
    case CSN_DEV_WIDE_GEMM: csn_gemm_wide = value; break;
    case CSN_DEV_WIDE_FORMS: csn_gemm_wide_set = value; break;
    case CSN_DEV_WX:
      if (value & ~(1 | 4 | 8)) return CSN_E_ARG;                   // only the bits of csn_hip.h: the setting stays as it was
      csn_dev_wx = value;
      break;
    case CSN_DEV_LNB_GROUP: csn_dev_lnb_group = value < 0 ? 0 : value; break;
    case CSN_DEV_SCONV_NB:
      if (value < 0 || value > 4) return CSN_E_ARG;
      csn_dev_sconv_nb = value;
      break;
    case CSN_DEV_KV_SAME:
      if (value != 0 && value != 1) return CSN_E_ARG;
      csn_dev_kv_same = value;
      break;
    case CSN_DEV_ATTN_WG64:
      if (value != 0 && value != 1) return CSN_E_ARG;
      csn_dev_attn_wg64 = value;
      break;
    case CSN_DEV_ATTN_WG64_LAUNCHES: return CSN_E_ARG;              // a counter: read-only
    default: return CSN_E_ARG;
  }
  return prev;
}

int csn_set_math_mode(int m) {
  if (m < 0 || m > 3) return CSN_E_ARG;
  g_math_mode = m;
  return 0;
}
int csn_set_thread_math_mode(int m) {
  if (m < -1 || m > 3) return CSN_E_ARG;
  t_math_mode = m;
  return 0;
}
int csn_get_math_mode(void) { return mode(); }
int csn_get_thread_math_mode(void) { return t_math_mode; }
int csn_set_thread_act16(int fmt) {
  if (fmt < 0 || (fmt & 3) == 3 || fmt > 6 || fmt == 4) return CSN_E_ARG;
  t_act16 = fmt;
  return 0;
}
int csn_get_thread_act16(void) { return t_act16; }
int csn_set_thread_rows16(int on) {
  if (on != 0 && on != 1) return CSN_E_ARG;
  t_rows16 = on;
  return 0;
}
int csn_get_thread_rows16(void) { return t_rows16; }
int csn_set_thread_score_layout(int layout) {
  if (layout < 0 || layout > 1) return CSN_E_ARG;
  t_score_layout = layout;
  return 0;
}
int csn_get_thread_score_layout(void) { return t_score_layout; }

const char* csn_status_string(int status) {
  switch (status) {
    case 0: return "ok";
    case CSN_E_ARG: return "csn: null pointer, non-positive size, a count beyond its row, or a flag this math mode does not take";
    case CSN_E_ALIGN: return "csn: a size or leading dimension is not a multiple of 4 floats";
    case CSN_E_PTR: return "csn: device pointer not 16-byte aligned";
    case CSN_E_STRIDE: return "csn: a stride is not a multiple of 4 floats";
    case CSN_E_DIM: return "csn: unsupported head / model dimension (need 32, 64, 96, 128 or 256)";
    case CSN_E_WORKSPACE: return "csn: workspace too small";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "csn: unknown status";
  }
}

long long csn_wgrad_workspace_floats(int rows, int cols, int n_maps, int n_points) {
  if (rows <= 0 || cols <= 0 || n_maps <= 0 || n_points <= 0) return 0;
  const int chunk = wgrad_chunk(n_maps, n_points);
  const long long n_chunks = (n_points + chunk - 1) / chunk;
  return (long long)n_maps * n_chunks * rows * cols;
}

int csn_project_f32(const float* x, long long x_shape_stride, int ld_x, const float* w, int rows, int channels,
                    float* out, long long out_shape_stride, int ld_out, int n_shapes, int n_points, int div_rows,
                    float temperature, int out_split, long long out_plane_stride, void* stream) {
  const int x16 = out_split >= 0 ? (out_split & 16) : 0;             // + 16: x is a bf16 map (math mode 2)
  if (out_split >= 0) out_split &= ~16;
  if (x16 && mode() != 2) return CSN_E_ARG;
  if (out_split && mode() == 0) return CSN_E_ARG;
  if (out_split < 0 || out_split > 3) return CSN_E_ARG;
  if (out_split == 3 && mode() < 2) return CSN_E_ARG;               // one 16-bit map: the single-product modes
  if (!x || !w || !out || rows <= 0 || channels <= 0 || n_shapes <= 0 || n_points <= 0) return CSN_E_ARG;
  if (out_split == 2) {
    // tile planes: out_plane_stride = points per attention block (<= 512), ld_out = row pitch = n_blocks * 512 * planes
    const int bp = 512 * planes_of(mode());
    if (out_plane_stride <= 0 || out_plane_stride > 512 || (out_plane_stride & 3) || (ld_out % bp)) return CSN_E_ARG;
    if (((long long)n_points + out_plane_stride - 1) / out_plane_stride * bp > ld_out) return CSN_E_ARG;
    if (out_shape_stride & 7) return CSN_E_STRIDE;
  }
  if (out_split == 1 && mode() != 1) return CSN_E_ARG;              // whole hi / lo planes: mode 1 only
  if (n_points > ld_x || (out_split != 2 && n_points > ld_out)) return CSN_E_ARG;      // a row holds the points it is read for
  if ((ld_x & 3) || (ld_out & 3) || (n_points & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(x) || mis16(w) || mis16(out)) return CSN_E_PTR;
  if ((x_shape_stride & 3) || (out_shape_stride & 3)) return CSN_E_STRIDE;
  if (mode() == 1 && !x16 && (out_split == 0 || out_split == 2) && !(div_rows & 31) && csn_wx_takes(rows, channels)) {
    const int rc = launch_wx(w, x, x_shape_stride, ld_x, out, out_shape_stride, ld_out, rows, n_shapes, n_points, div_rows, temperature,
                             out_split, (int)out_plane_stride, (hipStream_t)stream);
    if (rc != CSN_NOT_TAKEN) return rc;                               // (a geometry the stream does not take: the tiled kernel below)
  }
  CsnGemmArgs g;
  g.A = operand(w, 0, 0, 0, nullptr, channels);
  g.B = operand(x, 0, 0, x_shape_stride, nullptr, ld_x);
  if (x16) g.B.fmt = CSN_FMT_16;
  g.C = operand(out, 0, 0, out_shape_stride, nullptr, ld_out);
  g.C.planes = out_split == 3 ? 1 : out_split; g.C.plane_stride = out_plane_stride;
  g.M = rows; g.N = n_points; g.K = channels;
  g.n0 = 1; g.n1 = 1; g.k_chunk = 0;
  g.alpha = 1.f; g.div_rows = div_rows; g.div_val = temperature; g.accumulate = 0; g.eval_ids = nullptr;
  return launch_gemm(g, /*b_is_nk=*/0, n_shapes, (hipStream_t)stream);
}

int csn_project_qkv_f32(const float* x, long long x_shape_stride, int ld_x, const float* w_qkv, int d_inner, int channels,
                        float* q_out, long long q_shape_stride, int ld_q, void* kv_out, long long kv_shape_stride, int ld_kv,
                        int n_shapes, int n_points, float temperature, int block, void* stream) {
  if (!q_out || !kv_out || d_inner <= 0) return CSN_E_ARG;
  if (mode() == 0) return CSN_E_ARG;                                  // tile planes: the 16-bit modes
  // one pass over x where the streaming kernel takes the product (bf16x3, 256 channels, 256 rows each of Q, K, V) ...
  if (mode() == 1 && d_inner == 256 && csn_wx_takes(3 * d_inner, channels)) {
    if (!x || !w_qkv || channels <= 0 || n_shapes <= 0 || n_points <= 0) return CSN_E_ARG;
    const int bp = 512 * planes_of(mode());
    if (block <= 0 || block > 512 || (block & 3) || (ld_kv % bp)) return CSN_E_ARG;
    if (((long long)n_points + block - 1) / block * bp > ld_kv) return CSN_E_ARG;
    if (n_points > ld_x || n_points > ld_q) return CSN_E_ARG;
    if ((ld_x & 3) || (ld_q & 3) || (n_points & 3)) return CSN_E_ALIGN;
    if (mis16(x) || mis16(w_qkv) || mis16(q_out) || mis16(kv_out)) return CSN_E_PTR;
    if ((x_shape_stride & 3) || (q_shape_stride & 3) || (kv_shape_stride & 7)) return CSN_E_STRIDE;
    CsnWxArgs a;
    a.w = w_qkv; a.x = x; a.x_item_stride = x_shape_stride; a.ldx = ld_x;
    a.out = kv_out; a.out_item_stride = kv_shape_stride; a.ldo = ld_kv;
    a.out_f32 = q_out; a.out_f32_item_stride = q_shape_stride; a.ldo_f32 = ld_q; a.n_f32 = 1;
    a.n_items = n_shapes; a.n_points = n_points; a.n_sets = 3;
    a.div_rows = d_inner; a.div_val = temperature; a.div_rcp = 1.f / temperature;
    int ex = 0;
    a.div_exact = (std::frexp(temperature, &ex) == 0.5f && temperature > 0.f) ? 1 : 0;
    a.tb = block;
    const int rc = csn_launch_wx(a, 4, (hipStream_t)stream);
    if (rc != CSN_NOT_TAKEN) return rc;
  }
  // ... two projections elsewhere (the same results: an output element is one dot product in one order on either route)
  const int rc = csn_project_f32(x, x_shape_stride, ld_x, w_qkv, d_inner, channels, q_out, q_shape_stride, ld_q, n_shapes, n_points,
                                 d_inner, temperature, 0, 0, stream);
  if (rc) return rc;
  return csn_project_f32(x, x_shape_stride, ld_x, w_qkv + (long long)d_inner * channels, 2 * d_inner, channels,
                         static_cast<float*>(kv_out), kv_shape_stride, ld_kv, n_shapes, n_points, 0, 1.f, 2, block, stream);
}

// ---- (1b) folded projections ---------------------------------------------------------------------------------------------
// Exact fp32 whatever the thread's math mode: these are products of WEIGHTS (256^3, microseconds) whose rounding enters every
// score and every output of the step, so they go straight to the fp32 matrix-core GEMM, never through launch_gemm's mode switch.
static int gemm_exact(const float* a, int lda, const float* b, int ldb, int b_is_nk, float* c, int ldc, int M, int N, int K,
                      float div_val, hipStream_t st) {
  CsnGemmArgs g;
  g.A = operand(a, 0, 0, 0, nullptr, lda);
  g.B = operand(b, 0, 0, 0, nullptr, ldb);
  g.C = operand(c, 0, 0, 0, nullptr, ldc);
  g.M = M; g.N = N; g.K = K;
  g.n0 = 1; g.n1 = 1; g.k_chunk = 0;
  g.alpha = 1.f; g.div_rows = div_val != 1.f ? M : 0; g.div_val = div_val; g.accumulate = 0; g.eval_ids = nullptr;
  return csn_launch_gemm_f32(g, b_is_nk, 1, st);
}

long long csn_fold_workspace_floats(int d_inner, int channels) {
  return (d_inner <= 0 || channels <= 0) ? 0 : 2ll * d_inner * channels;
}

int csn_fold_weights_f32(const float* w_q, const float* w_k, const float* w_v, const float* w_fc, int d_inner, int channels,
                         float temperature, float* m, float* w_fv, float* w_fv_t, float* ws, long long ws_floats, void* stream) {
  if (!w_q || !w_k || !w_v || !w_fc || !m || !w_fv || !w_fv_t || !ws || d_inner <= 0 || channels <= 0) return CSN_E_ARG;
  if (!(temperature > 0.f)) return CSN_E_ARG;
  if ((d_inner & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(w_q) || mis16(w_k) || mis16(w_v) || mis16(w_fc) || mis16(m) || mis16(w_fv) || mis16(w_fv_t) || mis16(ws)) return CSN_E_PTR;
  if (ws_floats < csn_fold_workspace_floats(d_inner, channels)) return CSN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int D = d_inner, C = channels;
  float* wk_t = ws;                                  // [C][D]
  float* wv_t = ws + (long long)D * C;               // [C][D]
  CsnTransposeArgs t;
  t.src[0] = w_k; t.dst[0] = wk_t; t.src[1] = w_v; t.dst[1] = wv_t; t.src[2] = nullptr; t.dst[2] = nullptr;
  t.n = 2; t.rows = D; t.cols = C;
  int rc = csn_launch_transpose_f32(t, st);
  if (rc) return rc;
  rc = gemm_exact(wk_t, D, w_q, C, 0, m, C, C, C, D, temperature, st);          // M = W_k^T W_q / t
  if (rc) return rc;
  rc = gemm_exact(w_fc, D, w_v, C, 0, w_fv, C, C, C, D, 1.f, st);               // W_fv = W_fc W_v
  if (rc) return rc;
  return gemm_exact(wv_t, D, w_fc, D, 1, w_fv_t, C, C, C, D, 1.f, st);          // W_fv^T = W_v^T W_fc^T
}

int csn_unfold_wgrads_f32(const float* dm, const float* dw_fv, const float* w_q, const float* w_k, const float* w_v,
                          const float* w_fc, int d_inner, int channels, float temperature, float* dw_q, float* dw_k, float* dw_v,
                          float* dw_fc, float* ws, long long ws_floats, void* stream) {
  if (!dm || !dw_fv || !w_q || !w_k || !w_v || !w_fc || !dw_q || !dw_k || !dw_v || !dw_fc || !ws || d_inner <= 0 || channels <= 0)
    return CSN_E_ARG;
  if (!(temperature > 0.f)) return CSN_E_ARG;
  if ((d_inner & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(dm) || mis16(dw_fv) || mis16(w_q) || mis16(w_k) || mis16(w_v) || mis16(w_fc) || mis16(dw_q) || mis16(dw_k) ||
      mis16(dw_v) || mis16(dw_fc) || mis16(ws))
    return CSN_E_PTR;
  if (ws_floats < (long long)d_inner * channels) return CSN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int D = d_inner, C = channels;
  CsnTransposeArgs t;
  t.src[0] = w_fc; t.dst[0] = ws; t.src[1] = t.src[2] = nullptr; t.dst[1] = t.dst[2] = nullptr;      // W_fc^T [D][C]
  t.n = 1; t.rows = C; t.cols = D;
  int rc = csn_launch_transpose_f32(t, st);
  if (rc) return rc;
  rc = gemm_exact(w_k, C, dm, C, 0, dw_q, C, D, C, C, temperature, st);         // dW_q = W_k dM / t
  if (rc) return rc;
  rc = gemm_exact(w_q, C, dm, C, 1, dw_k, C, D, C, C, temperature, st);         // dW_k = W_q dM^T / t
  if (rc) return rc;
  rc = gemm_exact(dw_fv, C, w_v, C, 1, dw_fc, D, C, D, C, 1.f, st);             // dW_fc = dW_fv W_v^T
  if (rc) return rc;
  return gemm_exact(ws, C, dw_fv, C, 0, dw_v, C, D, C, C, 1.f, st);             // dW_v = W_fc^T dW_fv
}

int csn_tile_planes_f32(const float* x, long long x_shape_stride, int ld_x, void* out, long long out_shape_stride, int ld_out,
                        int n_shapes, int rows, int n_points, int block, void* stream) {
  if (!x || !out || n_shapes <= 0 || rows <= 0 || n_points <= 0) return CSN_E_ARG;
  if (block <= 0 || block > 512 || (ld_out % 1024)) return CSN_E_ARG;
  if (((long long)n_points + block - 1) / block * 1024 > ld_out || n_points > ld_x) return CSN_E_ARG;
  if (rows > 65535 || n_shapes > 65535) return CSN_E_ARG;
  if ((block & 3) || (ld_x & 3) || (n_points & 3)) return CSN_E_ALIGN;
  if (mis16(x) || mis16(out)) return CSN_E_PTR;
  if ((x_shape_stride & 3) || (out_shape_stride & 7)) return CSN_E_STRIDE;
  CsnTilePlanesArgs a;
  a.x = x; a.x_item_stride = x_shape_stride; a.ldx = ld_x;
  a.out = static_cast<short*>(out); a.out_item_stride = out_shape_stride; a.ldo = ld_out;
  a.n_items = n_shapes; a.rows = rows; a.n_points = n_points; a.tb = block;
  return csn_launch_tile_planes(a, (hipStream_t)stream);
}

static int attn_fwd_impl(const float* q, const float* k, const float* v, long long q_shape_stride,
                         long long kv_shape_stride, const int* q_index, const int* kv_index, int ld, float* ctx,
                         long long ctx_eval_stride, float* scores, float* lse, int n_evals, int n_heads,
                         int d_head, int block, int n_blocks, int score_pitch, float rescale_threshold,
                         float dropout_p, unsigned long long seed, int qkv_split, long long qkv_plane_stride,
                         int block_q, int ld_kv, void* stream, const int* tq_arr = nullptr, const int* t_arr = nullptr,
                         const int* eval_ids = nullptr, const int* group_offsets = nullptr, int n_groups = 0) {
  // block_q / ld_kv != 0: the queries of a block are counted separately from its keys (block = keys) and K/V maps have
  // their own leading dimension; key counts need not be multiples of 4 then (fp32 K/V maps only).  tq_arr / t_arr: the
  // per-evaluation counts of a ragged batch (block_q / block are then the maxima)
  const int bq = block_q > 0 ? block_q : block, lk = ld_kv > 0 ? ld_kv : ld;
  if (block_q < 0 || ld_kv < 0 || (ld_kv & 3)) return CSN_E_ARG;
  if (n_blocks <= 0 || block <= 0) return CSN_E_ARG;
  const int t_last = last_block_points(block, n_blocks, ld, block_q);
  if (t_last < 0) return t_last;
  if (block_q != 0 && (long long)n_blocks * ((block + 3) / 4 * 4) > lk) return CSN_E_ARG;
  if ((block & 3) && (block_q == 0 || qkv_split)) return CSN_E_ALIGN;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (qkv_split && mode() == 0) return CSN_E_ARG;
  if (!qkv_split && mode() >= 2) return CSN_E_ARG;                   // single-product modes take K / V as tile planes
  const int bp = 512 * planes_of(mode());
  if (qkv_split && (qkv_plane_stride <= 0 || (qkv_plane_stride % bp) || qkv_plane_stride < (long long)n_blocks * bp ||
                    block > 512 || (kv_shape_stride & 7)))
    return CSN_E_ARG;
  if (!q || !k || !v || !ctx || n_evals <= 0 || n_heads <= 0 || block <= 0 || n_blocks <= 0) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if ((ld & 3) || (score_pitch & 3) || score_pitch < (block + 3) / 4 * 4) return CSN_E_ALIGN;
  if (mis16(q) || mis16(k) || mis16(v) || mis16(ctx) || mis16(scores)) return CSN_E_PTR;
  if ((q_shape_stride & 3) || (kv_shape_stride & 3) || (ctx_eval_stride & 3)) return CSN_E_STRIDE;
  if (block_q != 0 && (long long)n_blocks * bq > ld) return CSN_E_ARG;
  CsnAttnArgs a;
  a.T_last = t_last;
  a.Tq = block_q; a.ld_kv = ld_kv;
  a.q = q; a.k = k; a.v = v;
  a.q_shape_stride = q_shape_stride; a.kv_shape_stride = kv_shape_stride;
  a.kv_ld = (int)qkv_plane_stride;
  a.q_index = q_index; a.kv_index = kv_index; a.ld = ld;
  a.out = ctx; a.out_eval_stride = ctx_eval_stride;
  a.scores = scores; a.dscores = nullptr; a.lse = lse; a.delta = nullptr; a.ctx = nullptr;
  a.E = n_evals; a.H = n_heads; a.T = block; a.Tp = score_pitch; a.n_blocks = n_blocks;
  a.rescale_threshold = rescale_threshold;
  a.eval_ids = eval_ids; a.grp_off = nullptr; a.out_index = nullptr; a.accumulate = 0;
  if (group_offsets) {                                               // grouped by query slot (16-bit modes; fp32: the listed evaluations, ungrouped)
    if (!eval_ids || n_groups <= 0 || n_groups > n_evals || block_q != 0 || tq_arr || t_arr) return CSN_E_ARG;
    if (mode() != 0) { a.grp_off = group_offsets; a.E = n_groups; }
  }
  a.dropout_p = dropout_p; a.seed = seed;
  a.r_planes = 0; a.kv_planes = qkv_split; a.r_plane_stride = 0; a.kv_plane_stride = 0; a.sc_tiles = 0;
  a.tq_arr = tq_arr; a.t_arr = t_arr;
  if (act16()) {                                                     // Qs in, Ctx out: 16-bit maps of the mode's type
    if (!act16_fwd_ok() || !qkv_split || block_q != 0) return CSN_E_ARG;
    a.r_fmt = a.out_fmt = act16();
  }
  if (t_score_layout && scores) {                                    // tile-major scores: block mode, bf16x3, tile-plane K / V
    if (mode() != 1 || !qkv_split || block_q != 0 || tq_arr || t_arr || score_pitch < (block + 31) / 32 * 32) return CSN_E_ARG;
    a.sc_layout = 1;
  }
  return mode() != 0 ? csn_launch_attn_fwd_bf16x3(a, d_head, mode(), (hipStream_t)stream)
                     : csn_launch_attn_fwd_f32(a, d_head, (hipStream_t)stream);
}

int csn_block_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                           long long kv_shape_stride, const int* q_index, const int* kv_index, int ld, float* ctx,
                           long long ctx_eval_stride, float* scores, float* lse, int n_evals, int n_heads,
                           int d_head, int block, int n_blocks, int score_pitch, float rescale_threshold,
                           float dropout_p, unsigned long long seed, int qkv_split, long long qkv_plane_stride,
                           void* stream) {
  return attn_fwd_impl(q, k, v, q_shape_stride, kv_shape_stride, q_index, kv_index, ld, ctx, ctx_eval_stride, scores, lse,
                       n_evals, n_heads, d_head, block, n_blocks, score_pitch, rescale_threshold, dropout_p, seed, qkv_split,
                       qkv_plane_stride, 0, 0, stream);
}

int csn_block_attn_fwd_grouped_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                                   long long kv_shape_stride, const int* q_index, const int* kv_index, int ld, float* ctx,
                                   long long ctx_eval_stride, float* scores, float* lse, int n_evals, int n_heads,
                                   int d_head, int block, int n_blocks, int score_pitch, float rescale_threshold,
                                   float dropout_p, unsigned long long seed, int qkv_split, long long qkv_plane_stride,
                                   const int* eval_ids, const int* group_offsets, int n_groups, void* stream) {
  if (!eval_ids || !group_offsets) return CSN_E_ARG;
  return attn_fwd_impl(q, k, v, q_shape_stride, kv_shape_stride, q_index, kv_index, ld, ctx, ctx_eval_stride, scores, lse,
                       n_evals, n_heads, d_head, block, n_blocks, score_pitch, rescale_threshold, dropout_p, seed, qkv_split,
                       qkv_plane_stride, 0, 0, stream, nullptr, nullptr, eval_ids, group_offsets, n_groups);
}

int csn_cross_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                           long long kv_shape_stride, int ld_q, int ld_kv, float* ctx, long long ctx_eval_stride,
                           float* scores, float* lse, int n_evals, int n_heads, int d_head, int n_queries, int n_keys,
                           int score_pitch, float rescale_threshold, float dropout_p, unsigned long long seed, void* stream) {
  if (n_queries <= 0 || n_keys <= 0) return CSN_E_ARG;
  if (n_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  return attn_fwd_impl(q, k, v, q_shape_stride, kv_shape_stride, nullptr, nullptr, ld_q, ctx, ctx_eval_stride, scores, lse,
                       n_evals, n_heads, d_head, n_keys, 1, score_pitch, rescale_threshold, dropout_p, seed, 0, 0, n_queries,
                       ld_kv, stream);
}

static int attn_bwd_dq_impl(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* k,
                            const float* v, long long kv_shape_stride, const int* kv_index, int ld, float* scores,
                            float* dscores, const float* lse, float* delta, float* dq, long long dq_slot_stride,
                            const int* dq_index, int accumulate, const int* eval_ids, int n_launch_evals, int n_heads,
                            int d_head, int block, int n_blocks, int score_pitch, float dropout_p,
                            unsigned long long seed, int dctx_split, long long dctx_plane_stride, int kv_split,
                            long long kv_plane_stride, int probs_tiles, int block_q, int ld_kv, const int* group_offsets,
                            int n_groups, void* stream, const int* tq_arr = nullptr, const int* t_arr = nullptr,
                            const float* q = nullptr, long long q_shape_stride = 0, const int* q_index = nullptr) {
  if (block_q < 0 || ld_kv < 0 || (ld_kv & 3)) return CSN_E_ARG;
  // q != NULL: the scores are recomputed from the pre-scaled queries (block mode, tile-plane K / V, where the kernel has room)
  if (q && (block_q != 0 || !kv_split || !(csn_attn_bwd_grouping(d_head, block) & 4) || mis16(q))) return CSN_E_ARG;
  if (q && (q_shape_stride & 3)) return CSN_E_STRIDE;
  if ((tq_arr || t_arr) && (group_offsets || n_blocks != 1)) return CSN_E_ARG;
  if (n_blocks <= 0 || block <= 0) return CSN_E_ARG;
  const int t_last = last_block_points(block, n_blocks, ld, block_q);
  if (t_last < 0) return t_last;
  if (block_q != 0 && ((long long)n_blocks * block_q > ld || (long long)n_blocks * ((block + 3) / 4 * 4) > (ld_kv > 0 ? ld_kv : ld)))
    return CSN_E_ARG;                                                 // cross-length: queries and keys fit their rows
  if (group_offsets && (n_groups <= 0 || !eval_ids || !(csn_attn_bwd_grouping(d_head, block) & 1))) return CSN_E_ARG;
  if ((block & 3) && (block_q == 0 || kv_split)) return CSN_E_ALIGN;
  if (probs_tiles && (mode() == 0 || score_pitch < (block + 31) / 32 * 32)) return CSN_E_ARG;
  // probs_tiles == 2: dS planes only, the scores stay untouched (kept scores, where the dV-from-scores kernel exists)
  // probs_tiles == 3: no planes at all — scores read-only, dscores unused (may be NULL); the same conditions
  if (probs_tiles < 0 || probs_tiles > 3) return CSN_E_ARG;
  if (probs_tiles >= 2 && (q || !kv_split || block_q != 0 || tq_arr || t_arr || act16() ||
                           !csn_attn_bwd_dv_scores_available(d_head, block)))
    return CSN_E_ARG;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (dctx_split) return CSN_E_ARG;                                  // reserved (see header)
  if (kv_split && mode() == 0) return CSN_E_ARG;
  if (kv_split < 0 || kv_split > 2 || (kv_split == 2 && mode() != 2)) return CSN_E_ARG;   // 2: fp16 planes of a mode-3 forward
  if (mode() == 3) return CSN_E_ARG;                                 // fp16: forward only — run the backward in mode 2
  if (mode() == 2 && !(kv_split && (probs_tiles || q))) return CSN_E_ARG;   // single-product mode: tile planes in and out
  const int bp = 512 * planes_of(mode());
  if (kv_split && (kv_plane_stride <= 0 || (kv_plane_stride % bp) || kv_plane_stride < (long long)n_blocks * bp ||
                   block > 512 || (kv_shape_stride & 7)))
    return CSN_E_ARG;
  // (recomputed scores with probs_tiles == 0: nothing is read from or written to scores / dscores — they may be NULL)
  // (recomputed scores in the one-plane mode: P and dS both travel in dscores, `scores` is never touched)
  const bool need_sc = !q || (probs_tiles && mode() == 1), need_ds = (!q || probs_tiles) && probs_tiles != 3;
  // (delta is an OUTPUT nobody has to want: NULL with probs_tiles == 3, where no dK / dV product follows that would read it)
  if (!dctx || !ctx || !k || !v || !lse || (!delta && probs_tiles != 3) || !dq || (need_sc && !scores) || (need_ds && !dscores)) return CSN_E_ARG;
  if (n_launch_evals <= 0 || n_heads <= 0 || block <= 0 || n_blocks <= 0) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if ((ld & 3) || (score_pitch & 3) || score_pitch < (block + 3) / 4 * 4) return CSN_E_ALIGN;
  if (mis16(dctx) || mis16(k) || mis16(v) || mis16(scores) || mis16(dscores) || mis16(dq)) return CSN_E_PTR;
  if ((kv_shape_stride & 3) || (ctx_eval_stride & 3) || (dq_slot_stride & 3)) return CSN_E_STRIDE;
  hipStream_t st = (hipStream_t)stream;
  // delta[e][h][n] = sum_c dctx * ctx (softmax backward row constant) is formed in the kernel's prologue, where
  // the dctx columns are being loaded anyway
  CsnAttnArgs a;
  a.ctx = ctx;
  a.T_last = t_last;
  a.Tq = block_q; a.ld_kv = ld_kv;
  a.q = dctx; a.k = k; a.v = v;
  a.q_shape_stride = dctx_split ? 2 * ctx_eval_stride : ctx_eval_stride;     // split dctx: [eval][2 planes][D][ld]
  a.kv_shape_stride = kv_shape_stride;
  a.q_index = nullptr; a.kv_index = kv_index; a.ld = ld;
  a.out = dq; a.out_eval_stride = dq_slot_stride;
  a.scores = scores; a.dscores = dscores; a.lse = const_cast<float*>(lse); a.delta = delta;
  a.E = group_offsets ? n_groups : n_launch_evals; a.H = n_heads; a.T = block; a.Tp = score_pitch; a.n_blocks = n_blocks;
  a.rescale_threshold = 0.f;
  a.eval_ids = eval_ids; a.grp_off = group_offsets; a.out_index = dq_index; a.accumulate = accumulate;
  a.dropout_p = dropout_p; a.seed = seed;
  a.r_planes = 0; a.kv_planes = kv_split != 0; a.r_plane_stride = 0; a.kv_plane_stride = 0; a.kv_ld = (int)kv_plane_stride;
  a.kv_f16 = kv_split == 2;
  a.sc_tiles = probs_tiles;
  // keys and values are the same tile planes (folded projections; one stride and one pitch describe both): one request per tile
  if (kv_split == 1 && k == v && mode() == 1 && d_head == 256 && probs_tiles == 3) a.kv_same = csn_dev_kv_same;
  a.tq_arr = tq_arr; a.t_arr = t_arr;
  a.q2 = q; a.q2_shape_stride = q_shape_stride; a.q2_index = q_index;
  if (t_score_layout) {                                              // tile-major scores in, tile-major P / dS planes out
    if (mode() != 1 || !kv_split || block_q != 0 || tq_arr || t_arr || !probs_tiles) return CSN_E_ARG;
    a.sc_layout = 1;
  }
  if (act16()) {                                                     // dO: bf16; O and Qs: the forward's 16-bit type; dQ stays fp32
    if (!act16_bwd_ok() || !kv_split || block_q != 0) return CSN_E_ARG;
    a.r_fmt = 1; a.ctx_fmt = act16(); a.q2_fmt = act16();
    if (grad16()) {
      if (accumulate) return CSN_E_ARG;                               // a 16-bit gradient map is written once (grouped calls)
      a.out_fmt = 1;
    }
  }
  return mode() != 0 ? csn_launch_attn_bwd_bf16x3(a, d_head, mode(), st) : csn_launch_attn_bwd_f32(a, d_head, st);
}

int csn_block_attn_bwd_dq_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* k,
                              const float* v, long long kv_shape_stride, const int* kv_index, int ld, float* scores,
                              float* dscores, const float* lse, float* delta, float* dq, long long dq_slot_stride,
                              const int* dq_index, int accumulate, const int* eval_ids, int n_launch_evals, int n_heads,
                              int d_head, int block, int n_blocks, int score_pitch, float dropout_p,
                              unsigned long long seed, int dctx_split, long long dctx_plane_stride, int kv_split,
                              long long kv_plane_stride, int probs_tiles, const int* group_offsets, int n_groups,
                              void* stream) {
  return attn_bwd_dq_impl(dctx, ctx, ctx_eval_stride, k, v, kv_shape_stride, kv_index, ld, scores, dscores, lse, delta, dq,
                          dq_slot_stride, dq_index, accumulate, eval_ids, n_launch_evals, n_heads, d_head, block, n_blocks,
                          score_pitch, dropout_p, seed, dctx_split, dctx_plane_stride, kv_split, kv_plane_stride, probs_tiles,
                          0, 0, group_offsets, n_groups, stream);
}

int csn_block_attn_bwd_dq_recompute_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q,
                                        long long q_shape_stride, const int* q_index, const float* k, const float* v,
                                        long long kv_shape_stride, const int* kv_index, int ld, float* probs,
                                        float* dscores, const float* lse, float* delta, float* dq,
                                        long long dq_slot_stride, const int* dq_index, int accumulate, const int* eval_ids,
                                        int n_launch_evals, int n_heads, int d_head, int block, int n_blocks,
                                        int score_pitch, float dropout_p, unsigned long long seed,
                                        long long kv_plane_stride, int kv_f16, int probs_tiles, const int* group_offsets,
                                        int n_groups, void* stream) {
  if (!q) return CSN_E_ARG;
  return attn_bwd_dq_impl(dctx, ctx, ctx_eval_stride, k, v, kv_shape_stride, kv_index, ld, probs, dscores, lse, delta, dq,
                          dq_slot_stride, dq_index, accumulate, eval_ids, n_launch_evals, n_heads, d_head, block, n_blocks,
                          score_pitch, dropout_p, seed, 0, 0, kv_f16 ? 2 : 1, kv_plane_stride, probs_tiles, 0, 0, group_offsets,
                          n_groups, stream, nullptr, nullptr, q, q_shape_stride, q_index);
}

static int attn_bwd_dkv_impl(const float* dctx, long long ctx_eval_stride, const float* q, long long q_shape_stride,
                             const int* q_index, int ld, const float* probs, const float* dscores, float* dk,
                             float* dv, long long dkv_slot_stride, const int* dk_index, const int* dv_index,
                             int accumulate, const int* eval_ids, int n_launch_evals, int n_heads, int d_head,
                             int block, int n_blocks, int score_pitch, int dctx_split, long long dctx_plane_stride,
                             int q_split, long long q_plane_stride, int probs_tiles, int block_q, int ld_kv,
                             const int* group_offsets, int n_groups, void* stream, const int* tq_arr = nullptr,
                             const int* t_arr = nullptr) {
  // block_q / ld_kv != 0 (cross-length attention): block counts the keys, block_q (% 4) the queries that are contracted;
  // dk / dv are [d][ld_kv] maps whose columns block .. round-up-4(block) are written as zeros
  if (block_q < 0 || ld_kv < 0 || (ld_kv & 3) || (block_q & 3)) return CSN_E_ARG;
  if ((block & 3) && block_q == 0) return CSN_E_ALIGN;
  const int bq = block_q > 0 ? block_q : block, lk = ld_kv > 0 ? ld_kv : ld, bk4 = (block + 3) / 4 * 4;
  if (n_blocks <= 0 || block <= 0) return CSN_E_ARG;
  const int t_last = last_block_points(block, n_blocks, ld, block_q);
  if (t_last < 0) return t_last;
  if (block_q != 0 && ((long long)n_blocks * bk4 > lk || (long long)n_blocks * bq > ld)) return CSN_E_ARG;
  if (probs_tiles && (mode() == 0 || score_pitch < (block + 31) / 32 * 32)) return CSN_E_ARG;
  if (mode() == 3 || (mode() == 2 && !probs_tiles)) return CSN_E_ARG;
  if (dctx_split || q_split) return CSN_E_ARG;                       // reserved (see header)
  if (group_offsets && (n_groups <= 0 || !eval_ids || !(csn_attn_bwd_grouping(d_head, block) & 2))) return CSN_E_ARG;
  // probs == NULL && dv == NULL: dK alone (the dV product is somebody else's: csn_block_attn_bwd_dv_scores_f32)
  const bool dk_only = !probs && !dv;
  if (!dctx || !q || !dscores || !dk || (!dv && !dk_only)) return CSN_E_ARG;
  if (!probs && !dk_only && !(probs_tiles && mode() == 2)) return CSN_E_ARG;   // (one plane: P and dS are both read from dscores)
  if (n_launch_evals <= 0 || n_heads <= 0 || block <= 0 || n_blocks <= 0) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if ((ld & 3) || (score_pitch & 3) || score_pitch < bk4) return CSN_E_ALIGN;
  if (mis16(dctx) || mis16(q) || mis16(probs) || mis16(dscores) || mis16(dk) || mis16(dv)) return CSN_E_PTR;
  if ((q_shape_stride & 3) || (ctx_eval_stride & 3) || (dkv_slot_stride & 3)) return CSN_E_STRIDE;
  hipStream_t st = (hipStream_t)stream;
  // dV^T[c][key] (+)= sum_q dO^T[c][q] P[q][key]   and   dK^T[d][key] (+)= sum_q Qs^T[d][q] dS[q][key]
  // (the score blocks are stored [query][key]: k-major B operands)
  const long long blk_sc = (long long)bq * score_pitch;
  CsnGemmArgs g;
  g.M = d_head; g.N = bk4; g.K = bq;
  g.n0 = n_blocks; g.n1 = n_heads; g.k_chunk = 0;
  g.alpha = 1.f; g.div_rows = 0; g.div_val = 1.f; g.accumulate = accumulate; g.eval_ids = eval_ids;
  if (group_offsets) { g.eval_ids = nullptr; g.grp_off = group_offsets; g.grp_items = eval_ids; }
  g.n_arr = t_arr; g.k_arr = tq_arr;            // ragged batch: keys (rounded up to 4 by the kernel) / queries of every evaluation
  g.n_last = g.k_last = t_last;                 // the row ends inside the last block
  const int n_batch = group_offsets ? n_groups : n_launch_evals;
  int rc = 0;
  if (act16() && (!act16_bwd_ok() || !probs_tiles || block_q != 0)) return CSN_E_ARG;
  g.A = operand(dctx, bq, (long long)d_head * ld, dctx_split ? 2 * ctx_eval_stride : ctx_eval_stride, nullptr, ld);
  g.A.planes = dctx_split; g.A.plane_stride = dctx_plane_stride;
  if (act16()) g.A.fmt = CSN_FMT_16;                                 // dO: a bf16 map
  // tile planes: the same buffers viewed as 16-bit elements (two per float: block strides double).  Two planes (mode 1): a
  // row of 16 tiles [hi | lo] is the fp32 row, pitch 2 * score_pitch, P in `probs`, dS in `dscores`.  One plane (mode 2):
  // compact rows of pitch score_pitch, both in `dscores` — per block [P: bq rows | dS: bq rows] (`probs` is not read)
  const int bm = probs_tiles ? 2 : 1;
  const bool one_plane = probs_tiles && mode() == 2;
  const int ldb = one_plane ? score_pitch : bm * score_pitch;
  const float* p_src = one_plane ? dscores : probs;
  const float* ds_src = one_plane ? reinterpret_cast<const float*>(reinterpret_cast<const short*>(dscores) + blk_sc) : dscores;
  // tile-major P / dS planes (csn_set_thread_score_layout): where the dV / dK products run on the 16-wave 256 x 256 kernel
  const bool tile_major = t_score_layout != 0;
  if (tile_major && (mode() != 1 || !probs_tiles || block_q != 0 || tq_arr || t_arr || !csn_gemm_tile_major_planes(d_head, bk4)))
    return CSN_E_ARG;
  g.B = operand(p_src, bm * blk_sc, bm * blk_sc * n_blocks, bm * blk_sc * n_blocks * n_heads, nullptr, ldb);
  g.B.planes = probs_tiles ? (tile_major ? 3 : 2) : 0;
  const bool g16 = act16() && grad16();
  if (g16 && accumulate) return CSN_E_ARG;                            // a 16-bit gradient map is written once (grouped calls)
  g.C = operand(dv, block, (long long)d_head * lk, dkv_slot_stride, dv_index, lk);
  if (g16) g.C.planes = 1;
  if (!dk_only) rc = launch_gemm(g, 0, n_blocks * n_heads * n_batch, st);
  if (rc) return rc;
  g.A = operand(q, bq, (long long)d_head * ld, q_shape_stride, q_index, ld);
  g.A.planes = q_split; g.A.plane_stride = q_plane_stride;
  if (act16()) g.A.fmt = act16() == 2 ? CSN_FMT_F16_TO_BF16 : CSN_FMT_16;   // Qs: the forward's 16-bit map
  g.B = operand(ds_src, bm * blk_sc, bm * blk_sc * n_blocks, bm * blk_sc * n_blocks * n_heads, nullptr, ldb);
  g.B.planes = probs_tiles ? (tile_major ? 3 : 2) : 0;
  g.C = operand(dk, block, (long long)d_head * lk, dkv_slot_stride, dk_index, lk);
  if (g16) g.C.planes = 1;
  return launch_gemm(g, 0, n_blocks * n_heads * n_batch, st);
}

int csn_block_attn_bwd_dkv_f32(const float* dctx, long long ctx_eval_stride, const float* q, long long q_shape_stride,
                               const int* q_index, int ld, const float* probs, const float* dscores, float* dk,
                               float* dv, long long dkv_slot_stride, const int* dk_index, const int* dv_index,
                               int accumulate, const int* eval_ids, int n_launch_evals, int n_heads, int d_head,
                               int block, int n_blocks, int score_pitch, int dctx_split, long long dctx_plane_stride,
                               int q_split, long long q_plane_stride, int probs_tiles, const int* group_offsets,
                               int n_groups, void* stream) {
  return attn_bwd_dkv_impl(dctx, ctx_eval_stride, q, q_shape_stride, q_index, ld, probs, dscores, dk, dv, dkv_slot_stride,
                           dk_index, dv_index, accumulate, eval_ids, n_launch_evals, n_heads, d_head, block, n_blocks,
                           score_pitch, dctx_split, dctx_plane_stride, q_split, q_plane_stride, probs_tiles, 0, 0,
                           group_offsets, n_groups, stream);
}

int csn_attn_bwd_grouping(int d_head, int block) {
  if (mode() == 0) return 0;
  const bool tiles_ok = mode() != 3 && block <= 512 && !(block & 3) && dim_ok(d_head);
  const bool recompute = tiles_ok && csn_attn_recompute_fits(planes_of(mode()), d_head / 32);
  const bool flash = recompute && csn_attn_dkv_flash_fits(d_head / 32);
  const bool tm = mode() == 1 && tiles_ok && csn_gemm_tile_major_planes(d_head, (block + 3) / 4 * 4);
  return 1 | (csn_gemm_bf16x3_big_tiles(d_head, (block + 3) / 4 * 4) ? 2 : 0) | (recompute ? 4 : 0) | (flash ? 8 : 0) | (tm ? 16 : 0);
}

int csn_attn_bwd_dv_scores_available(int d_head, int block) {
  return block > 0 && block <= 512 && !(block & 3) && csn_attn_dv_scores_fits(mode(), d_head);
}
// probs_tiles = 3 of the dq call: built beside the probs_tiles = 2 instance, for the same geometries
int csn_attn_bwd_dq_no_planes_available(int d_head, int block) { return csn_attn_bwd_dv_scores_available(d_head, block); }

int csn_block_attn_bwd_dv_scores_f32(const float* dctx, long long ctx_eval_stride, int ld, const float* scores, const float* lse,
                                     float* dv, long long dkv_slot_stride, const int* dv_index, const int* eval_ids,
                                     int n_launch_evals, int n_heads, int d_head, int block, int n_blocks, int score_pitch,
                                     float dropout_p, unsigned long long seed, const int* group_offsets, int n_groups,
                                     void* stream) {
  if (!dctx || !scores || !lse || !dv) return CSN_E_ARG;
  if (n_launch_evals <= 0 || n_heads <= 0 || block <= 0 || n_blocks <= 0) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if (!csn_attn_bwd_dv_scores_available(d_head, block)) return CSN_E_ARG;
  if (group_offsets && (n_groups <= 0 || !eval_ids)) return CSN_E_ARG;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (act16()) return CSN_E_ARG;                                      // fp32 scores, fp32 maps
  if (t_score_layout && (!(csn_attn_bwd_grouping(d_head, block) & 16) || score_pitch < (block + 31) / 32 * 32)) return CSN_E_ARG;
  const int t_last = last_block_points(block, n_blocks, ld, 0);
  if (t_last < 0) return t_last;
  if ((ld & 3) || (score_pitch & 3) || score_pitch < block) return CSN_E_ALIGN;
  if (mis16(dctx) || mis16(scores) || mis16(dv)) return CSN_E_PTR;
  if ((ctx_eval_stride & 3) || (dkv_slot_stride & 3)) return CSN_E_STRIDE;
  CsnAttnDvArgs a;
  a.dctx = dctx; a.ctx_eval_stride = ctx_eval_stride;
  a.scores = scores; a.lse = lse;
  a.dv = dv; a.dkv_slot_stride = dkv_slot_stride; a.dv_index = dv_index;
  a.eval_ids = eval_ids; a.grp_off = group_offsets; a.n_groups = group_offsets ? n_groups : n_launch_evals;
  a.ld = ld; a.H = n_heads; a.T = block; a.Tp = score_pitch; a.n_blocks = n_blocks; a.T_last = t_last;
  a.dropout_p = dropout_p; a.seed = seed;
  a.sc_layout = t_score_layout != 0;
  return csn_launch_attn_dv_scores(a, d_head, mode(), (hipStream_t)stream);
}

int csn_block_attn_bwd_dkv_flash_f32(const float* dctx, long long ctx_eval_stride, const float* q, long long q_shape_stride,
                                     const int* q_index, const float* k, const float* v, long long kv_shape_stride,
                                     const int* kv_index, long long kv_plane_stride, int kv_f16, int ld, const float* lse,
                                     const float* delta, float* dk, float* dv, long long dkv_slot_stride,
                                     const int* dk_index, const int* dv_index, int accumulate, const int* eval_ids,
                                     int n_launch_evals, int n_heads, int d_head, int block, int n_blocks, int score_pitch,
                                     float dropout_p, unsigned long long seed, const int* group_offsets, int n_groups,
                                     void* stream) {
  if (!dctx || !q || !k || !v || !lse || !delta || !dk || !dv) return CSN_E_ARG;
  if (n_launch_evals <= 0 || n_heads <= 0 || block <= 0 || n_blocks <= 0) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if (!(csn_attn_bwd_grouping(d_head, block) & 8)) return CSN_E_ARG;
  if (group_offsets && (n_groups <= 0 || !eval_ids)) return CSN_E_ARG;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (kv_f16 && mode() != 2) return CSN_E_ARG;
  const int t_last = last_block_points(block, n_blocks, ld, 0);
  if (t_last < 0) return t_last;
  const int bp = 512 * planes_of(mode());
  if (kv_plane_stride <= 0 || (kv_plane_stride % bp) || kv_plane_stride < (long long)n_blocks * bp || (kv_shape_stride & 7))
    return CSN_E_ARG;
  if ((ld & 3) || (score_pitch & 3) || score_pitch < block) return CSN_E_ALIGN;
  if (mis16(dctx) || mis16(q) || mis16(k) || mis16(v) || mis16(dk) || mis16(dv)) return CSN_E_PTR;
  if ((q_shape_stride & 3) || (ctx_eval_stride & 3) || (dkv_slot_stride & 3)) return CSN_E_STRIDE;
  CsnAttnDkvArgs a;
  a.q = q; a.q_shape_stride = q_shape_stride; a.q_index = q_index;
  a.dctx = dctx; a.ctx_eval_stride = ctx_eval_stride;
  a.k = k; a.v = v; a.kv_shape_stride = kv_shape_stride; a.kv_ld = (int)kv_plane_stride; a.kv_index = kv_index;
  a.lse = lse; a.delta = delta;
  a.dk = dk; a.dv = dv; a.dkv_slot_stride = dkv_slot_stride; a.dk_index = dk_index; a.dv_index = dv_index;
  a.accumulate = accumulate;
  a.eval_ids = eval_ids; a.grp_off = group_offsets; a.n_groups = group_offsets ? n_groups : n_launch_evals;
  a.ld = ld; a.H = n_heads; a.T = block; a.Tp = score_pitch; a.n_blocks = n_blocks; a.T_last = t_last;
  a.dropout_p = dropout_p; a.seed = seed; a.kv_f16 = kv_f16 != 0;
  if (act16()) {
    if (!act16_bwd_ok()) return CSN_E_ARG;
    a.q_fmt = act16(); a.dctx_fmt = 1;
    if (grad16()) {
      if (accumulate) return CSN_E_ARG;
      a.out_fmt = 1;
    }
  }
  return csn_launch_attn_dkv_flash(a, d_head, mode(), (hipStream_t)stream);
}

/* cross-length attention backward (MinkowskiNet/models/attention.py: one unchunked block per evaluation, n_queries != n_keys;
 * gradients flow to queries, keys and values).  n_queries % 4 == 0 (pad with zero points); n_keys arbitrary. */
int csn_cross_attn_bwd_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                           const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                           float* scores, float* dscores, const float* lse, float* delta, float* dq, float* dk, float* dv,
                           long long dq_eval_stride, long long dkv_eval_stride, int n_evals, int n_heads, int d_head,
                           int n_queries, int n_keys, int score_pitch, float dropout_p, unsigned long long seed,
                           void* stream) {
  if (n_queries <= 0 || n_keys <= 0) return CSN_E_ARG;
  if (n_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  const int pt = (mode() != 0 && score_pitch >= (n_keys + 31) / 32 * 32) ? 1 : 0;
  int rc = attn_bwd_dq_impl(dctx, ctx, ctx_eval_stride, k, v, kv_shape_stride, nullptr, ld_q, scores, dscores, lse, delta, dq,
                            dq_eval_stride, nullptr, 0, nullptr, n_evals, n_heads, d_head, n_keys, 1, score_pitch, dropout_p,
                            seed, 0, 0, 0, 0, pt, n_queries, ld_kv, nullptr, 0, stream);
  if (rc) return rc;
  return attn_bwd_dkv_impl(dctx, ctx_eval_stride, q, q_shape_stride, nullptr, ld_q, scores, dscores, dk, dv, dkv_eval_stride,
                           nullptr, nullptr, 0, nullptr, n_evals, n_heads, d_head, n_keys, 1, score_pitch, 0, 0, 0, 0, pt,
                           n_queries, ld_kv, nullptr, 0, stream);
}

/* ragged batches of the cross-length attention: the same kernels with per-evaluation query / key counts (device arrays) */
int csn_varlen_attn_fwd_f32(const float* q, const float* k, const float* v, long long q_shape_stride,
                            long long kv_shape_stride, int ld_q, int ld_kv, float* ctx, long long ctx_eval_stride,
                            float* scores, float* lse, int n_evals, int n_heads, int d_head, int max_queries, int max_keys,
                            const int* n_queries, const int* n_keys, int score_pitch, float rescale_threshold,
                            float dropout_p, unsigned long long seed, void* stream) {
  if (max_queries <= 0 || max_keys <= 0 || !n_queries || !n_keys) return CSN_E_ARG;
  if (max_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  return attn_fwd_impl(q, k, v, q_shape_stride, kv_shape_stride, nullptr, nullptr, ld_q, ctx, ctx_eval_stride, scores, lse,
                       n_evals, n_heads, d_head, max_keys, 1, score_pitch, rescale_threshold, dropout_p, seed, 0, 0, max_queries,
                       ld_kv, stream, n_queries, n_keys);
}

int csn_varlen_attn_bwd_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                            const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                            float* scores, float* dscores, const float* lse, float* delta, float* dq, float* dk, float* dv,
                            long long dq_eval_stride, long long dkv_eval_stride, int n_evals, int n_heads, int d_head,
                            int max_queries, int max_keys, const int* n_queries, const int* n_keys, int score_pitch,
                            float dropout_p, unsigned long long seed, void* stream) {
  if (max_queries <= 0 || max_keys <= 0 || !n_queries || !n_keys) return CSN_E_ARG;
  if (max_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  const int pt = (mode() != 0 && score_pitch >= (max_keys + 31) / 32 * 32) ? 1 : 0;
  int rc = attn_bwd_dq_impl(dctx, ctx, ctx_eval_stride, k, v, kv_shape_stride, nullptr, ld_q, scores, dscores, lse, delta, dq,
                            dq_eval_stride, nullptr, 0, nullptr, n_evals, n_heads, d_head, max_keys, 1, score_pitch, dropout_p,
                            seed, 0, 0, 0, 0, pt, max_queries, ld_kv, nullptr, 0, stream, n_queries, n_keys);
  if (rc) return rc;
  return attn_bwd_dkv_impl(dctx, ctx_eval_stride, q, q_shape_stride, nullptr, ld_q, scores, dscores, dk, dv, dkv_eval_stride,
                           nullptr, nullptr, 0, nullptr, n_evals, n_heads, d_head, max_keys, 1, score_pitch, 0, 0, 0, 0, pt,
                           max_queries, ld_kv, nullptr, 0, stream, n_queries, n_keys);
}

/* the score-free backward of (3b) / (3c): the dQ kernel rebuilds S = Qs K^T from the fp32 K / V maps tile by tile and writes
 * delta and dQ, the key-stationary kernel rebuilds P and dS from lse and delta and writes dK and dV; both draw the forward's
 * dropout mask with the pitch max(n_queries, score_pitch).  Math mode 1 (modes 2 / 3 run as mode 1), d_head <= 128. */
static bool cross_flash_fits(int m, int d_head) {
  return m == 1 && dim_ok(d_head) && csn_attn_recompute_fits(2, d_head / 32) && csn_attn_dkv_flash_fits(d_head / 32);
}

int csn_cross_attn_flash_available(int d_head) { return cross_flash_fits(mode() >= 2 ? 1 : mode(), d_head) ? 1 : 0; }

static int cross_bwd_flash_impl(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                                const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                                const float* lse, float* delta, float* dq, float* dk, float* dv, long long dq_eval_stride,
                                long long dkv_eval_stride, int n_evals, int n_heads, int d_head, int n_queries, int n_keys,
                                const int* tq_arr, const int* t_arr, int score_pitch, float dropout_p, unsigned long long seed,
                                void* stream) {
  if (!dctx || !ctx || !q || !k || !v || !lse || !delta || !dq || !dk || !dv) return CSN_E_ARG;
  if (n_evals <= 0 || n_heads <= 0 || ld_q <= 0 || ld_kv <= 0) return CSN_E_ARG;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (!dim_ok(d_head)) return CSN_E_DIM;
  if (!cross_flash_fits(mode(), d_head)) return CSN_E_ARG;          // exact fp32, or a width no recomputing kernel has room for
  const int nk4 = (n_keys + 3) / 4 * 4;
  if (n_queries > ld_q || nk4 > ld_kv) return CSN_E_ARG;            // queries and keys fit their rows
  if ((ld_q & 3) || (ld_kv & 3) || (score_pitch & 3) || score_pitch < nk4) return CSN_E_ALIGN;
  if (mis16(dctx) || mis16(ctx) || mis16(q) || mis16(k) || mis16(v) || mis16(dq) || mis16(dk) || mis16(dv)) return CSN_E_PTR;
  if ((q_shape_stride & 3) || (kv_shape_stride & 3) || (ctx_eval_stride & 3) || (dq_eval_stride & 3) || (dkv_eval_stride & 3))
    return CSN_E_STRIDE;
  hipStream_t st = (hipStream_t)stream;
  CsnAttnArgs a{};
  a.q = dctx; a.k = k; a.v = v; a.ctx = ctx;
  a.q_shape_stride = ctx_eval_stride; a.kv_shape_stride = kv_shape_stride;
  a.ld = ld_q; a.ld_kv = ld_kv;
  a.out = dq; a.out_eval_stride = dq_eval_stride;
  a.lse = const_cast<float*>(lse); a.delta = delta;
  a.E = n_evals; a.H = n_heads; a.T = n_keys; a.Tq = n_queries; a.Tp = score_pitch; a.n_blocks = 1;
  a.dropout_p = dropout_p; a.seed = seed;
  a.tq_arr = tq_arr; a.t_arr = t_arr;
  a.q2 = q; a.q2_shape_stride = q_shape_stride;                      // (scores, dscores: NULL — nothing score-sized is read or written)
  int rc = csn_launch_attn_bwd_bf16x3(a, d_head, 1, st);
  if (rc) return rc;
  CsnAttnDkvArgs b{};
  b.q = q; b.q_shape_stride = q_shape_stride;
  b.dctx = dctx; b.ctx_eval_stride = ctx_eval_stride;
  b.k = k; b.v = v; b.kv_shape_stride = kv_shape_stride;
  b.lse = lse; b.delta = delta;
  b.dk = dk; b.dv = dv; b.dkv_slot_stride = dkv_eval_stride;
  b.n_groups = n_evals;
  b.ld = ld_q; b.ld_kv = ld_kv; b.H = n_heads; b.T = n_keys; b.Tq = n_queries; b.Tp = score_pitch; b.n_blocks = 1;
  b.dropout_p = dropout_p; b.seed = seed;
  b.tq_arr = tq_arr; b.t_arr = t_arr;
  return csn_launch_attn_dkv_flash(b, d_head, 1, st);
}

int csn_cross_attn_bwd_flash_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                                 const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                                 const float* lse, float* delta, float* dq, float* dk, float* dv, long long dq_eval_stride,
                                 long long dkv_eval_stride, int n_evals, int n_heads, int d_head, int n_queries, int n_keys,
                                 int score_pitch, float dropout_p, unsigned long long seed, void* stream) {
  if (n_queries <= 0 || n_keys <= 0) return CSN_E_ARG;
  if (n_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  return cross_bwd_flash_impl(dctx, ctx, ctx_eval_stride, q, k, v, q_shape_stride, kv_shape_stride, ld_q, ld_kv, lse, delta, dq,
                              dk, dv, dq_eval_stride, dkv_eval_stride, n_evals, n_heads, d_head, n_queries, n_keys, nullptr,
                              nullptr, score_pitch, dropout_p, seed, stream);
}

int csn_varlen_attn_bwd_flash_f32(const float* dctx, const float* ctx, long long ctx_eval_stride, const float* q, const float* k,
                                  const float* v, long long q_shape_stride, long long kv_shape_stride, int ld_q, int ld_kv,
                                  const float* lse, float* delta, float* dq, float* dk, float* dv, long long dq_eval_stride,
                                  long long dkv_eval_stride, int n_evals, int n_heads, int d_head, int max_queries, int max_keys,
                                  const int* n_queries, const int* n_keys, int score_pitch, float dropout_p,
                                  unsigned long long seed, void* stream) {
  if (max_queries <= 0 || max_keys <= 0 || !n_queries || !n_keys) return CSN_E_ARG;
  if (max_queries & 3) return CSN_E_ALIGN;
  ModeGuard guard(mode() >= 2 ? 1 : mode());
  return cross_bwd_flash_impl(dctx, ctx, ctx_eval_stride, q, k, v, q_shape_stride, kv_shape_stride, ld_q, ld_kv, lse, delta, dq,
                              dk, dv, dq_eval_stride, dkv_eval_stride, n_evals, n_heads, d_head, max_queries, max_keys, n_queries,
                              n_keys, score_pitch, dropout_p, seed, stream);
}

long long csn_masked_ce_workspace_bytes(int n_shapes, int n_points) {
  if (n_shapes <= 0 || n_points <= 0) return 0;
  return csn_masked_ce_blocks(n_shapes, n_points) * 3 * (long long)sizeof(double);
}

int csn_masked_ce_fwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels, long long label_shape_stride,
                          int n_shapes, int n_classes, int n_points, int mask, float* lse, void* ws, long long ws_bytes,
                          float* stats, void* stream) {
  if (!logits || !labels || !lse || !ws || !stats || n_shapes <= 0 || n_classes <= 0 || n_points <= 0 || n_points > ld) return CSN_E_ARG;
  if (n_shapes > 65535 || n_classes > 65535) return CSN_E_DIM;
  if (reinterpret_cast<unsigned long long>(ws) & 7) return CSN_E_PTR;
  if (ws_bytes < csn_masked_ce_workspace_bytes(n_shapes, n_points)) return CSN_E_WORKSPACE;
  CsnMaskedCeArgs a{};
  a.logits = logits; a.shape_stride = shape_stride; a.ld = ld; a.labels = labels; a.label_shape_stride = label_shape_stride;
  a.n_shapes = n_shapes; a.n_classes = n_classes; a.n_points = n_points; a.mask = mask;
  a.lse = lse; a.partials = static_cast<double*>(ws); a.stats = stats;
  return csn_launch_masked_ce_fwd(a, (hipStream_t)stream);
}

long long csn_masked_ce_metrics_workspace_bytes(int n_shapes, int n_classes, int n_points) {
  if (n_classes <= 0) return 0;
  return csn_masked_ce_workspace_bytes(n_shapes, n_points);
}

int csn_masked_ce_metrics_fwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels,
                                  long long label_shape_stride, int n_shapes, int n_classes, int n_points, int mask, float* lse,
                                  int* pred, int* counts, void* ws, long long ws_bytes, float* stats, void* stream) {
  if (!logits || !labels || !counts || !ws || !stats || n_shapes <= 0 || n_classes <= 0 || n_points <= 0 || n_points > ld) return CSN_E_ARG;
  if (n_shapes > 65535 || n_classes > 65535) return CSN_E_DIM;
  if (reinterpret_cast<unsigned long long>(ws) & 7) return CSN_E_PTR;
  if (ws_bytes < csn_masked_ce_metrics_workspace_bytes(n_shapes, n_classes, n_points)) return CSN_E_WORKSPACE;
  CsnMaskedCeArgs a{};
  a.logits = logits; a.shape_stride = shape_stride; a.ld = ld; a.labels = labels; a.label_shape_stride = label_shape_stride;
  a.n_shapes = n_shapes; a.n_classes = n_classes; a.n_points = n_points; a.mask = mask;
  a.lse = lse; a.pred = pred; a.counts = counts; a.partials = static_cast<double*>(ws); a.stats = stats;
  return csn_launch_masked_ce_fwd(a, (hipStream_t)stream);
}

int csn_masked_ce_bwd_f32(const float* logits, long long shape_stride, int ld, const long long* labels, long long label_shape_stride,
                          int n_shapes, int n_classes, int n_points, int mask, const float* lse, const float* stats,
                          const float* grad_out, float* dlogits, long long dshape_stride, int dld, void* stream) {
  if (!logits || !labels || !lse || !stats || !grad_out || !dlogits || n_shapes <= 0 || n_classes <= 0 || n_points <= 0 || n_points > ld ||
      n_points > dld)
    return CSN_E_ARG;
  if (n_shapes > 65535 || n_classes > 65535) return CSN_E_DIM;
  // (any point count, pitch and alignment, like the forward: the launcher takes the 16-byte form where the geometry allows it)
  CsnMaskedCeArgs a{};
  a.logits = logits; a.shape_stride = shape_stride; a.ld = ld; a.labels = labels; a.label_shape_stride = label_shape_stride;
  a.n_shapes = n_shapes; a.n_classes = n_classes; a.n_points = n_points; a.mask = mask;
  a.lse = const_cast<float*>(lse); a.stats = const_cast<float*>(stats); a.grad_out = grad_out;
  a.dlogits = dlogits; a.dshape_stride = dshape_stride; a.dld = dld;
  return csn_launch_masked_ce_bwd(a, (hipStream_t)stream);
}

long long csn_outproj_ln_workspace_floats(int n_evals, int d_model, int d_inner, int n_points) {
  if (n_evals <= 0 || d_model <= 0 || d_inner <= 0 || n_points <= 0) return 0;
  const long long tiled = (long long)n_evals * ((n_points + 255) / 256) * d_model;
  const long long stream = d_model == 256 && d_inner == 256 ? (long long)n_evals * csn_wx_ln_sum_slots(n_evals, n_points) * 256 : 0;
  return tiled > stream ? tiled : stream;
}

int csn_outproj_ln_fwd_f32(const float* ctx, long long ctx_eval_stride, const float* wfc, const float* xres,
                           long long xres_shape_stride, const int* res_index, float* xhat,
                           long long xhat_eval_stride, float* rstd, int n_evals, int d_model, int d_inner, int ld,
                           int n_points, float eps, float dropout_p, unsigned long long seed, float* xhat_sum,
                           float* sum_ws, long long sum_ws_floats, void* stream) {
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (!ctx || !wfc || !xres || !xhat || !rstd || n_evals <= 0 || n_points <= 0 || d_inner <= 0 || n_points > ld) return CSN_E_ARG;
  if (dropout_p > 0.f && (long long)(d_model / 2 + 1) * ld >= (1ll << 32)) return CSN_E_ARG;   // 32-bit mask pair index
  if (xhat_sum && xhat_eval_stride != (long long)d_model * ld) return CSN_E_STRIDE;     // the row-sum pass walks dense maps
  if (!dim_ok(d_model)) return CSN_E_DIM;
  if ((ld & 3) || (d_inner & 3) || (n_points & 3)) return CSN_E_ALIGN;
  if (mis16(ctx) || mis16(wfc) || mis16(xres) || mis16(xhat)) return CSN_E_PTR;
  if ((ctx_eval_stride & 3) || (xres_shape_stride & 3) || (xhat_eval_stride & 3)) return CSN_E_STRIDE;
  CsnOutProjArgs a;
  a.ctx = ctx; a.ctx_eval_stride = ctx_eval_stride; a.wfc = wfc;
  a.xres = xres; a.xres_shape_stride = xres_shape_stride; a.res_index = res_index;
  a.xhat = xhat; a.xhat_eval_stride = xhat_eval_stride; a.rstd = rstd;
  a.E = n_evals; a.C = d_model; a.D = d_inner; a.ld = ld; a.n_points = n_points; a.eps = eps;
  a.dropout_p = dropout_p; a.seed = seed;
  a.xhat_sum = xhat_sum; a.sum_ws = sum_ws; a.sum_ws_floats = sum_ws ? sum_ws_floats : 0;
  if (act16() && !act16_fwd_ok()) return CSN_E_ARG;
  a.act16 = act16();
  return csn_launch_outproj_ln_fwd_f32(a, mode(), (hipStream_t)stream);
}

int csn_outproj_ln_bwd_f32(const float* dxhat, const float* xhat, const float* rstd, long long eval_stride,
                           const float* ctx, long long ctx_eval_stride, const float* wfc_t, float* dz, float* dz_res,
                           float* dctx, float* dwfc, float* ws, long long ws_floats, int n_evals, int d_model,
                           int d_inner, int ld, int n_points, int accumulate, float dropout_p,
                           unsigned long long seed, int dctx_split, long long dctx_plane_stride,
                           const float* dxhat_rows, int n_dense_evals, const float* dxhat_scale, int dxhat_group,
                           void* stream) {
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (dxhat_group < 0) return CSN_E_ARG;
  if (dropout_p > 0.f && (long long)(d_model / 2 + 1) * ld >= (1ll << 32)) return CSN_E_ARG;   // 32-bit mask pair index
  if (dctx_split && mode() == 0) return CSN_E_ARG;
  if (n_dense_evals < 0 || n_dense_evals > n_evals || (n_dense_evals > 0 && !dxhat)) return CSN_E_ARG;
  if (!xhat || !rstd || !ctx || !wfc_t || !dz || !dctx || !dwfc || !ws) return CSN_E_ARG;
  if (n_evals <= 0 || n_points <= 0 || d_inner <= 0 || d_model <= 0 || n_points > ld) return CSN_E_ARG;
  if ((ld & 3) || (d_inner & 3) || (d_model & 3) || (n_points & 3)) return CSN_E_ALIGN;
  if (mis16(dxhat) || mis16(xhat) || mis16(ctx) || mis16(wfc_t) || mis16(dz) || mis16(dctx) || mis16(dwfc) || mis16(ws))
    return CSN_E_PTR;
  if ((eval_stride & 3) || (ctx_eval_stride & 3)) return CSN_E_STRIDE;
  hipStream_t st = (hipStream_t)stream;
  CsnLnBwdArgs l;
  l.dxhat = dxhat; l.xhat = xhat; l.rstd = rstd; l.dz = dz; l.dz_res = dz_res; l.eval_stride = eval_stride;
  l.E = n_evals; l.C = d_model; l.ld = ld; l.n_points = n_points;
  l.dropout_p = dropout_p; l.seed = seed;
  l.dxhat_rows = dxhat_rows; l.n_dense = n_dense_evals;
  l.dxhat_scale = dxhat_scale; l.dxhat_group = dxhat_group > 0 ? dxhat_group : 1;
  const int a16 = act16();
  if (a16 && (!act16_bwd_ok() || dctx_split)) return CSN_E_ARG;
  l.act16 = a16;
  int rc = 0;
  // dctx[e][D][n] = wfc_t[D][c] dz[e][c][n]
  if (mode() == 1 && !a16 && !dctx_split && csn_wx_takes(d_inner, d_model) &&
      csn_wx_geometry_takes(csn_dev_lnb_group > 0 && csn_dev_lnb_group < n_evals ? csn_dev_lnb_group : n_evals, n_points, d_inner / 256)) {
    // (development switch CSN_DEV_LNB_GROUP = G > 0: LayerNorm backward and dCtx alternate over groups of G evaluations, so that a
    //  group's dz is read back while it may still sit in the 256 MB Infinity Cache)
    const int G = csn_dev_lnb_group > 0 ? csn_dev_lnb_group : n_evals;
    const bool fused = csn_wx_lnb_takes(l, d_inner) && eval_stride == ctx_eval_stride;
    for (int e0 = 0; e0 < n_evals && !rc; e0 += G) {
      const int ng = n_evals - e0 < G ? n_evals - e0 : G;
      if (fused) {                                       // one pass: xhat in, dz (and dz_res) and dCtx out (wx_lnb.hip)
        CsnWxLnbArgs f{};
        f.w = wfc_t; f.xhat = xhat; f.rstd = rstd; f.eval_stride = eval_stride; f.ld = ld;
        f.dxhat = dxhat; f.dxhat_group = l.dxhat_group; f.n_dense = n_dense_evals; f.dxhat_scale = dxhat_scale; f.dxhat_rows = dxhat_rows;
        f.dz = dz; f.dz_res = dz_res; f.dctx = dctx; f.dctx_eval_stride = ctx_eval_stride;
        f.n_items = ng; f.n_points = n_points; f.e_base = e0; f.dropout_p = dropout_p; f.seed = seed;
        rc = csn_launch_wx_lnb(f, st);
        if (rc != CSN_NOT_TAKEN) continue;
      }
      l.e_base = e0; l.E = ng;
      rc = csn_launch_ln_bwd_f32(l, st);
      if (rc) return rc;
      rc = launch_wx(wfc_t, dz + (long long)e0 * eval_stride, eval_stride, ld, dctx + (long long)e0 * ctx_eval_stride, ctx_eval_stride, ld,
                     d_inner, ng, n_points, 0, 1.f, 0, 0, st);
    }
    if (rc) return rc;
    return wgrad(dz, eval_stride, ld, ctx, ctx_eval_stride, ld, dwfc, d_model, d_inner, n_evals, n_points, 1.f, accumulate, ws,
                 ws_floats, st, 0, 0);
  }
  rc = csn_launch_ln_bwd_f32(l, st);
  if (rc) return rc;
  CsnGemmArgs g;
  g.A = operand(wfc_t, 0, 0, 0, nullptr, d_model);
  g.B = operand(dz, 0, 0, eval_stride, nullptr, ld);
  g.C = operand(dctx, 0, 0, dctx_split ? 2 * ctx_eval_stride : ctx_eval_stride, nullptr, ld);   // split: [eval][2][D][ld]
  g.C.planes = dctx_split; g.C.plane_stride = dctx_plane_stride;
  if (a16) { g.B.fmt = CSN_FMT_16; g.C.planes = 1; }                 // dz in, dctx out: bf16 maps
  g.M = d_inner; g.N = n_points; g.K = d_model;
  g.n0 = 1; g.n1 = 1; g.k_chunk = 0;
  g.alpha = 1.f; g.div_rows = 0; g.div_val = 1.f; g.accumulate = 0; g.eval_ids = nullptr;
  rc = launch_gemm(g, 0, n_evals, st);
  if (rc) return rc;
  // dwfc[c][D] (+)= sum_{e,n} dz[e][c][n] ctx[e][D][n]
  return wgrad(dz, eval_stride, ld, ctx, ctx_eval_stride, ld, dwfc, d_model, d_inner, n_evals, n_points, 1.f,
               accumulate, ws, ws_floats, st, a16 ? CSN_FMT_16 : 0, a16 == 2 ? CSN_FMT_F16_TO_BF16 : (a16 ? CSN_FMT_16 : 0));
}

// the evaluations e_base .. e_base + n_evals - 1 on the fused kernel (wx_lnb.hip), or none at all
static bool lnb_range_takes(int n_evals, int d_model, int d_inner, int ld, int n_points, long long eval_stride) {
  if (n_evals <= 0 || n_points <= 0 || n_points > ld || mode() != 1 || act16()) return false;
  CsnLnBwdArgs l{};
  l.C = d_model; l.ld = ld; l.n_points = n_points; l.eval_stride = eval_stride; l.act16 = 0;
  return csn_wx_takes(d_inner, d_model) && csn_wx_geometry_takes(n_evals, n_points, d_inner / 256) && csn_wx_lnb_takes(l, d_inner);
}

long long csn_outproj_lnb_workspace_floats(int n_evals, int d_model, int d_inner, int ld, int n_points) {
  if (!lnb_range_takes(n_evals, d_model, d_inner, ld, n_points, (long long)d_model * ld)) return 0;
  return csn_wx_lnb_red_floats(n_evals, n_points);
}

int csn_outproj_lnb_f32(const float* dxhat, const float* xhat, const float* rstd, long long eval_stride, const float* wfc_t,
                        float* dz, float* dz_res, float* dctx, int e_base, int n_evals, int d_model, int d_inner, int ld,
                        int n_points, float dropout_p, unsigned long long seed, const float* dxhat_rows, int n_dense_evals,
                        const float* dxhat_scale, int dxhat_group, float* rowdot, float* rowsum, float* red_ws,
                        long long red_ws_floats, void* stream) {
  if (dropout_p < 0.f || dropout_p >= 1.f) return CSN_E_ARG;
  if (dxhat_group < 0 || e_base < 0 || n_evals <= 0 || n_dense_evals < 0 || (n_dense_evals > 0 && !dxhat)) return CSN_E_ARG;
  if (!xhat || !rstd || !wfc_t || !dz || !dctx) return CSN_E_ARG;
  if (n_points <= 0 || d_inner <= 0 || d_model <= 0 || n_points > ld) return CSN_E_ARG;
  if (dropout_p > 0.f && (long long)(d_model / 2 + 1) * ld >= (1ll << 32)) return CSN_E_ARG;   // 32-bit mask pair index
  if ((ld & 3) || (d_inner & 3) || (d_model & 3) || (n_points & 3)) return CSN_E_ALIGN;
  if (mis16(dxhat) || mis16(xhat) || mis16(wfc_t) || mis16(dz) || mis16(dz_res) || mis16(dctx) || mis16(red_ws)) return CSN_E_PTR;
  if (eval_stride & 3) return CSN_E_STRIDE;
  if (!lnb_range_takes(e_base + n_evals, d_model, d_inner, ld, n_points, eval_stride)) return CSN_E_DIM;
  const int group = dxhat_group > 0 ? dxhat_group : 1;
  const bool reduce = rowdot || rowsum || red_ws;
  if (reduce) {
    // the reductions: over a launch of whole groups of dense evaluations from evaluation 0 on
    if (!rowdot || !rowsum || !red_ws || e_base != 0 || n_evals > n_dense_evals || n_evals % group) return CSN_E_ARG;
    if (red_ws_floats < csn_wx_lnb_red_floats(n_evals, n_points)) return CSN_E_WORKSPACE;
  }
  CsnWxLnbArgs f{};
  f.w = wfc_t; f.xhat = xhat; f.rstd = rstd; f.eval_stride = eval_stride; f.ld = ld;
  f.dxhat = dxhat; f.dxhat_group = group; f.n_dense = n_dense_evals; f.dxhat_scale = dxhat_scale; f.dxhat_rows = dxhat_rows;
  f.dz = dz; f.dz_res = dz_res; f.dctx = dctx; f.dctx_eval_stride = eval_stride;
  f.n_items = n_evals; f.n_points = n_points; f.e_base = e_base; f.dropout_p = dropout_p; f.seed = seed;
  if (reduce) { f.red_ws = red_ws; f.red_slots = csn_wx_ln_sum_slots(n_evals, n_points); f.rowdot = rowdot; f.rowsum = rowsum; }
  const int rc = csn_launch_wx_lnb(f, (hipStream_t)stream);
  return rc == CSN_NOT_TAKEN ? CSN_E_DIM : rc;
}

int csn_project_wgrad_f32(const float* dout, long long dout_shape_stride, int ld_dout, const float* x,
                          long long x_shape_stride, int ld_x, float* dw, int rows, int channels, int n_shapes,
                          int n_points, float scale, int accumulate, float* ws, long long ws_floats,
                          void* stream) {
  if (!dout || !x || !dw || !ws || rows <= 0 || channels <= 0 || n_shapes <= 0 || n_points <= 0) return CSN_E_ARG;
  if (n_points > ld_dout || n_points > ld_x) return CSN_E_ARG;
  // channels: the N of the product and the row pitch of every slab, written in 16-byte chunks (rows are only guarded per row)
  if ((ld_dout & 3) || (ld_x & 3) || (n_points & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(dout) || mis16(x) || mis16(dw) || mis16(ws)) return CSN_E_PTR;
  if ((dout_shape_stride & 3) || (x_shape_stride & 3)) return CSN_E_STRIDE;
  const bool g16 = act16() && grad16();                               // dout: bf16 gradient maps
  if (g16 && !act16_bwd_ok()) return CSN_E_ARG;
  return wgrad(dout, dout_shape_stride, ld_dout, x, x_shape_stride, ld_x, dw, rows, channels, n_shapes, n_points, scale,
               accumulate, ws, ws_floats, (hipStream_t)stream, g16 ? CSN_FMT_16 : 0, 0);
}

int csn_retrieval_measure_f32(const float* f1, const float* f2, float* out, int s1, int n1, int s2, int n2,
                              int channels, float* ws, long long ws_floats, void* stream) {
  if (!f1 || !f2 || !out || !ws || s1 <= 0 || s2 <= 0 || n1 <= 0 || n2 <= 0 || channels <= 0) return CSN_E_ARG;
  if (channels & 3) return CSN_E_ALIGN;
  if (mis16(f1) || mis16(f2) || mis16(ws)) return CSN_E_PTR;
  const long long need = (long long)s1 * n1 + (long long)s2 * n2 + (long long)s1 * s2 * n1;
  if (ws_floats < need) return CSN_E_WORKSPACE;
  return csn_launch_retrieval_f32(f1, f2, out, s1, n1, s2, n2, channels, ws, (hipStream_t)stream);
}

int csn_rowsum_f32(const float* x, float* out, long long rows, int n_points, long long ld, void* stream) {
  if (!x || !out || rows <= 0 || n_points <= 0 || n_points > ld) return CSN_E_ARG;
  if ((n_points & 3) || (ld & 3)) return CSN_E_ALIGN;
  if (mis16(x)) return CSN_E_PTR;
  return csn_launch_rowsum_f32(x, out, rows, n_points, ld, (hipStream_t)stream, act16());
}

int csn_mix_fwd_f32(const float* xhat, const float* comp, const float* gamma, const float* beta, float* feats,
                    int n_shapes, int k1, int channels, int n_points, const float* xhat_self, void* stream) {
  if (!comp || !gamma || !beta || !feats || n_shapes <= 0 || k1 <= 0 || k1 > 8 || channels <= 0 || n_points <= 0)
    return CSN_E_ARG;
  if (!xhat && !(xhat_self && k1 == 1)) return CSN_E_ARG;
  if (n_points & 3) return CSN_E_ALIGN;
  if (mis16(xhat) || mis16(feats) || mis16(xhat_self)) return CSN_E_PTR;
  return csn_launch_mix_fwd_f32(xhat, comp, gamma, beta, feats, n_shapes, k1, channels, n_points, xhat_self,
                                (hipStream_t)stream, act16());
}

int csn_mix_bwd_f32(const float* dfeats, const float* xhat, const float* comp, const float* gamma, float* dxhat,
                    float* rowdot, float* rowsum, int n_shapes, int k1, int channels, int n_points, const float* xhat_self,
                    float* dxhat_self, void* stream) {
  if (!dfeats || !comp || !gamma || !rowdot || !rowsum) return CSN_E_ARG;
  if (!xhat && !(xhat_self && k1 == 1)) return CSN_E_ARG;
  // gradient maps: all of them or none (none = reductions only; csn_outproj_ln_bwd_f32 then rebuilds them from dfeats)
  const bool want_maps = xhat_self ? dxhat_self != nullptr : dxhat != nullptr;
  if (want_maps && xhat_self && xhat && !dxhat) return CSN_E_ARG;
  if (!want_maps && (dxhat || dxhat_self)) return CSN_E_ARG;
  if (dxhat_self && !xhat_self) return CSN_E_ARG;                     // a gradient map for own-shape maps that were not given
  if (n_shapes <= 0 || k1 <= 0 || k1 > 8 || channels <= 0 || n_points <= 0) return CSN_E_ARG;
  if (n_points & 3) return CSN_E_ALIGN;
  if (mis16(dfeats) || mis16(xhat) || mis16(dxhat) || mis16(xhat_self) || mis16(dxhat_self)) return CSN_E_PTR;
  if (act16() && want_maps) return CSN_E_ARG;                         // fp16 maps: the linked form (reductions only)
  return csn_launch_mix_bwd_f32(dfeats, xhat, comp, gamma, dxhat, rowdot, rowsum, n_shapes, k1, channels, n_points, xhat_self,
                                dxhat_self, (hipStream_t)stream, act16());
}

int csn_compat_fwd_f32(const float* pooled, const float* wq_t, const float* bq, const float* wk_t, const float* bk, float* comp,
                       double* save_u, double* save_norm, int n_shapes, int k1, int channels, int reference_layout, void* stream) {
  if (!pooled || !wq_t || !bq || !wk_t || !bk || !comp || !save_u || !save_norm) return CSN_E_ARG;
  if (n_shapes <= 0 || k1 <= 0 || k1 > 8 || channels <= 0 || channels > 256) return CSN_E_ARG;
  return csn_launch_compat_fwd(pooled, wq_t, bq, wk_t, bk, comp, save_u, save_norm, n_shapes, k1, channels, reference_layout,
                               (hipStream_t)stream);
}

int csn_compat_bwd_f32(const float* dcomp, const float* comp, const double* save_u, const double* save_norm, const float* pooled,
                       const float* wq, const float* wk, double* ws, long long ws_doubles, float* dpooled, float* dwq, float* dbq,
                       float* dwk, float* dbk, int n_shapes, int k1, int channels, int reference_layout, void* stream) {
  if (!dcomp || !comp || !save_u || !save_norm || !pooled || !wq || !wk || !ws || !dpooled || !dwq || !dbq || !dwk || !dbk)
    return CSN_E_ARG;
  if (n_shapes <= 0 || k1 <= 0 || k1 > 8 || channels <= 0 || channels > 256) return CSN_E_ARG;
  const long long rows = (long long)n_shapes * (k1 + 1) * channels;
  if (ws_doubles < 2 * rows) return CSN_E_WORKSPACE;
  return csn_launch_compat_bwd(dcomp, comp, save_u, save_norm, pooled, wq, wk, ws, ws + rows, dpooled, dwq, dbq, dwk, dbk, n_shapes,
                               k1, channels, reference_layout, (hipStream_t)stream);
}

// ---- (11) ragged MinkowskiNet head ----
// offsets [n + 1]: offsets[0] == 0, strictly increasing (every shape >= 1 point); returns the longest shape, or -1
static long long ragged_offsets_max(const int* off, int n) {
  if (!off || n <= 0 || off[0] != 0) return -1;
  long long mx = 0;
  for (int i = 0; i < n; ++i) {
    if (off[i + 1] <= off[i]) return -1;
    mx = off[i + 1] - off[i] > mx ? off[i + 1] - off[i] : mx;
  }
  return mx;
}

static bool ragged_maps_ok(long long eval_stride, int ld, int channels) {
  return ld > 0 && channels > 0 && eval_stride >= (long long)channels * ld;
}

int csn_ragged_pool_f32(const float* xhat, long long eval_stride, int ld, const int* counts_host, const int* counts,
                        int n_evals, int channels, const float* gamma, const float* beta, float* pooled, float* mean, void* stream) {
  if (!xhat || !counts_host || !counts || !gamma || !beta || !pooled || n_evals <= 0) return CSN_E_ARG;
  if (!ragged_maps_ok(eval_stride, ld, channels)) return CSN_E_ARG;
  for (int e = 0; e < n_evals; ++e)
    if (counts_host[e] < 1 || counts_host[e] > ld) return CSN_E_ARG;
  if ((ld & 3) || (eval_stride & 3)) return CSN_E_ALIGN;
  if (mis16(xhat)) return CSN_E_PTR;
  return csn_launch_ragged_pool_f32(xhat, eval_stride, ld, counts, n_evals, channels, gamma, beta, pooled, mean, (hipStream_t)stream);
}

int csn_ragged_pool_bwd_f32(const float* dpooled, const float* gamma, const int* counts_host, const int* counts, int n_evals,
                            int channels, float* dxhat, long long eval_stride, int ld, int accumulate, void* stream) {
  if (!dpooled || !gamma || !counts_host || !counts || !dxhat || n_evals <= 0 || accumulate < 0 || accumulate > 1) return CSN_E_ARG;
  if (!ragged_maps_ok(eval_stride, ld, channels)) return CSN_E_ARG;
  for (int e = 0; e < n_evals; ++e)
    if (counts_host[e] < 1 || counts_host[e] > ld) return CSN_E_ARG;
  if ((ld & 3) || (eval_stride & 3)) return CSN_E_ALIGN;
  if (mis16(dxhat)) return CSN_E_PTR;
  return csn_launch_ragged_pool_bwd_f32(dpooled, gamma, counts, n_evals, channels, dxhat, eval_stride, ld, accumulate,
                                        (hipStream_t)stream);
}

// the mixed evaluations ev(b, j) lie inside [0, n_evals) and the cross ones after the shapes' own
static bool ragged_mix_evals_ok(int n_evals, int cross_first, int n_shapes, int k1) {
  if (n_shapes > n_evals) return false;
  if (k1 == 1) return true;
  return cross_first >= n_shapes && (long long)cross_first + (long long)(k1 - 1) * n_shapes <= n_evals;
}

int csn_ragged_mix_fwd_f32(const float* xhat, long long eval_stride, int ld, int n_evals, int cross_first,
                           const int* offsets_host, const int* offsets, int n_shapes, int k1, int channels, const float* comp,
                           const float* gamma, const float* beta, float* out, long long ld_out, void* stream) {
  if (!xhat || !offsets || !comp || !gamma || !beta || !out || n_shapes <= 0 || k1 <= 0 || k1 > 8) return CSN_E_ARG;
  if (!ragged_maps_ok(eval_stride, ld, channels) || ld_out < channels) return CSN_E_ARG;
  if (!ragged_mix_evals_ok(n_evals, cross_first, n_shapes, k1)) return CSN_E_ARG;
  const long long mx = ragged_offsets_max(offsets_host, n_shapes);
  if (mx < 1 || mx > ld) return CSN_E_ARG;
  if ((ld & 3) || (eval_stride & 3) || (ld_out & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(xhat) || mis16(out)) return CSN_E_PTR;
  return csn_launch_ragged_mix_fwd_f32(xhat, eval_stride, ld, cross_first, offsets, n_shapes, k1, channels, (int)mx, comp, gamma, beta,
                                       out, ld_out, (hipStream_t)stream);
}

int csn_ragged_mix_bwd_f32(const float* dout, long long ld_dout, const float* xhat, long long eval_stride, int ld, int n_evals,
                           int cross_first, const int* offsets_host, const int* offsets, int n_shapes, int k1, int channels,
                           const float* comp, const float* gamma, float* dxhat, double* rowdot, double* rowsum, double* ws,
                           long long ws_doubles, void* stream) {
  if (!dout || !xhat || !offsets || !comp || !gamma || !dxhat || !rowdot || !rowsum || !ws) return CSN_E_ARG;
  if (n_shapes <= 0 || k1 <= 0 || k1 > 8) return CSN_E_ARG;
  if (!ragged_maps_ok(eval_stride, ld, channels) || ld_dout < channels) return CSN_E_ARG;
  if (!ragged_mix_evals_ok(n_evals, cross_first, n_shapes, k1)) return CSN_E_ARG;
  const long long mx = ragged_offsets_max(offsets_host, n_shapes);
  if (mx < 1 || mx > ld) return CSN_E_ARG;
  if ((ld & 3) || (eval_stride & 3) || (ld_dout & 3) || (channels & 3)) return CSN_E_ALIGN;
  if (mis16(dout) || mis16(xhat) || mis16(dxhat)) return CSN_E_PTR;
  if (ws_doubles < (long long)n_shapes * (k1 + 1) * csn_ragged_mix_tiles(ld) * channels) return CSN_E_WORKSPACE;
  return csn_launch_ragged_mix_bwd_f32(dout, ld_dout, xhat, eval_stride, ld, cross_first, offsets, n_shapes, k1, channels, comp, gamma,
                                       dxhat, rowdot, rowsum, ws, (hipStream_t)stream);
}

int csn_ragged_retrieval_f32(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                             const int* offsets2_host, const int* offsets2, int s2, int channels, float* out, float* ws,
                             long long ws_floats, void* stream) {
  if (!f1 || !f2 || !offsets1 || !offsets2 || !out || !ws || s1 <= 0 || s2 <= 0 || channels <= 0) return CSN_E_ARG;
  const long long mx1 = ragged_offsets_max(offsets1_host, s1), mx2 = ragged_offsets_max(offsets2_host, s2);
  if (mx1 < 1 || mx2 < 1) return CSN_E_ARG;
  if ((long long)s1 * s2 > 0x7fffffffLL) return CSN_E_ARG;
  if (channels & 3) return CSN_E_ALIGN;
  if (mis16(f1) || mis16(f2) || mis16(ws)) return CSN_E_PTR;
  const long long N1 = offsets1_host[s1], N2 = offsets2_host[s2];
  const long long need = N1 + N2 + (long long)s1 * s2 * ((mx1 + 127) / 128);
  if (ws_floats < need) return CSN_E_WORKSPACE;
  return csn_launch_ragged_retrieval_f32(f1, offsets1, s1, N1, f2, offsets2, s2, N2, (int)mx1, channels, out, ws, (hipStream_t)stream);
}

// ---- (11b) fp16 screen and pair-list form of the ragged retrieval measure ----
static int ragged_retrieval_args(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                                 const int* offsets2_host, const int* offsets2, int s2, int channels, const float* out, const float* ws,
                                 long long* mx1) {
  if (!f1 || !f2 || !offsets1 || !offsets2 || !out || !ws || s1 <= 0 || s2 <= 0 || channels <= 0) return CSN_E_ARG;
  *mx1 = ragged_offsets_max(offsets1_host, s1);
  if (*mx1 < 1 || ragged_offsets_max(offsets2_host, s2) < 1) return CSN_E_ARG;
  if ((long long)s1 * s2 > 0x7fffffffLL) return CSN_E_ARG;
  if (channels & 3) return CSN_E_ALIGN;
  if (mis16(f1) || mis16(f2) || mis16(ws)) return CSN_E_PTR;
  return 0;
}

long long csn_retrieval_screen_workspace_floats(long long n1_rows, long long n2_rows, int s1, int s2, int max_n1, int channels) {
  if (n1_rows <= 0 || n2_rows <= 0 || s1 <= 0 || s2 <= 0 || max_n1 <= 0 || channels <= 0) return 0;
  return (n1_rows + n2_rows) * (csn_screen_padded_channels(channels) / 2) + (long long)s1 * s2 * ((max_n1 + 127) / 128);
}

int csn_ragged_retrieval_screen_f16(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                                    const int* offsets2_host, const int* offsets2, int s2, int channels, float* out, float* ws,
                                    long long ws_floats, void* stream) {
  long long mx1 = 0;
  const int bad = ragged_retrieval_args(f1, offsets1_host, offsets1, s1, f2, offsets2_host, offsets2, s2, channels, out, ws, &mx1);
  if (bad) return bad;
  if (csn_screen_padded_channels(channels) > CSN_SCREEN_MAX_CP) return CSN_E_DIM;
  const long long N1 = offsets1_host[s1], N2 = offsets2_host[s2];
  if (ws_floats < csn_retrieval_screen_workspace_floats(N1, N2, s1, s2, (int)mx1, channels)) return CSN_E_WORKSPACE;
  return csn_launch_ragged_retrieval_screen_f16(f1, offsets1, s1, N1, f2, offsets2, s2, N2, (int)mx1, channels, out, ws,
                                                (hipStream_t)stream);
}

int csn_ragged_retrieval_pairs_f32(const float* f1, const int* offsets1_host, const int* offsets1, int s1, const float* f2,
                                   const int* offsets2_host, const int* offsets2, int s2, int channels, const int* pairs,
                                   long long n_pairs, float* out, float* ws, long long ws_floats, void* stream) {
  long long mx1 = 0;
  const int bad = ragged_retrieval_args(f1, offsets1_host, offsets1, s1, f2, offsets2_host, offsets2, s2, channels, out, ws, &mx1);
  if (bad) return bad;
  if (!pairs || n_pairs <= 0 || ((uintptr_t)pairs & 3)) return CSN_E_ARG;
  const long long N1 = offsets1_host[s1], N2 = offsets2_host[s2];
  if (ws_floats < N1 + N2 + n_pairs * ((mx1 + 127) / 128)) return CSN_E_WORKSPACE;
  return csn_launch_ragged_retrieval_pairs_f32(f1, offsets1, s1, N1, f2, offsets2, s2, N2, (int)mx1, channels, pairs, n_pairs, out, ws,
                                               (hipStream_t)stream);
}

// |screen - exact| <= eps for every pair (derivation: DESIGN.md "fp16 screen of the shape graph"; tests/retrieval_screen_ref.py
// restates it).  u = 2^-24 (fp32), h = 2^-11 (fp16), Cp = channels padded to 32.
float csn_retrieval_screen_eps(int channels) {
  if (channels <= 0) return 0.f;
  const double C = channels, Cp = csn_screen_padded_channels(channels);
  const double u = 1.0 / 16777216.0, h = 1.0 / 2048.0;
  const double d = h + (C + 8.0) * u;                                // one image element against the real unit row, relative
  const double operands = 2.0 * d + d * d;                           // both operands, Cauchy-Schwarz on unit rows
  const double subnormal = 2.0 * (1.0 / 2097152.0) * sqrt(Cp) * (1.0 + d);   // |element| < 2^-21 of a unit row: flushed or kept
  const double accumulate = Cp * 2.0 * u * (1.0 + d) * (1.0 + d);    // fp32 accumulation in the matrix unit, any order, truncating
  const double exact_path = (2.0 * C + 8.0) * u;                     // the fp32 measure against real arithmetic
  const double means = 256.0 * u;                                    // both means: fp32 trees of <= 61 000 points per shape, fp64 tile sums
  const double eps = (operands + subnormal + accumulate + exact_path + means) * (1.0 + 1.0 / 1048576.0);
  float e = (float)eps;
  if ((double)e < eps) e = nextafterf(e, 1.f);
  return e;
}

// ---- (12) loss, predictions and IoU counts of the MinkowskiNet head ----
long long csn_ragged_seg_workspace_bytes(int n_rows) {
  if (n_rows <= 0) return 0;
  return csn_ragged_seg_blocks(n_rows) * 4 * (long long)sizeof(double);
}

static int ragged_seg_dims(int n_rows, int ld, int n_classes) {
  if (n_rows <= 0 || n_classes < 2 || ld < n_classes) return CSN_E_ARG;
  if (n_rows > 0x7fffffff - 256 || ld > (1 << 20)) return CSN_E_DIM;       // 32-bit row indices; 256 rows below a 2 GiB window
  return 0;
}

int csn_ragged_seg_fwd_f32(const float* logits, int n_rows, int ld, const long long* labels, const int* offsets_host,
                           const int* offsets, int n_segments, int n_classes, int ignore_label, float* lse, float* nll, int* pred,
                           double* stats, int* counts, void* ws, long long ws_bytes, void* stream) {
  if (!logits || !labels || !offsets || !lse || !nll || !pred || !stats || !counts || !ws) return CSN_E_ARG;
  if (const int e = ragged_seg_dims(n_rows, ld, n_classes)) return e;
  if (ragged_offsets_max(offsets_host, n_segments) < 1 || offsets_host[n_segments] != n_rows) return CSN_E_ARG;
  if ((long long)n_segments * n_classes * 3 > 0x7fffffffLL) return CSN_E_DIM;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(stats) & 7)) return CSN_E_PTR;
  if (ws_bytes < csn_ragged_seg_workspace_bytes(n_rows)) return CSN_E_WORKSPACE;
  CsnRaggedSegArgs a{};
  a.logits = logits; a.n_rows = n_rows; a.ld = ld; a.labels = labels; a.offsets = offsets; a.n_segments = n_segments;
  a.n_classes = n_classes; a.ignore_label = ignore_label; a.lse = lse; a.nll = nll; a.pred = pred; a.stats = stats; a.counts = counts;
  a.partials = static_cast<double*>(ws);
  return csn_launch_ragged_seg_fwd(a, (hipStream_t)stream);
}

int csn_ragged_seg_bwd_f32(const float* logits, int n_rows, int ld, const long long* labels, int n_classes, int ignore_label,
                           const float* lse, const float* nll, const double* stats, const float* grad_out, float* dlogits, int dld,
                           void* stream) {
  if (!logits || !labels || !lse || !nll || !stats || !grad_out || !dlogits) return CSN_E_ARG;
  if (const int e = ragged_seg_dims(n_rows, ld, n_classes)) return e;
  if (const int e = ragged_seg_dims(n_rows, dld, n_classes)) return e;
  if (reinterpret_cast<uintptr_t>(stats) & 7) return CSN_E_PTR;
  CsnRaggedSegArgs a{};
  a.logits = logits; a.n_rows = n_rows; a.ld = ld; a.labels = labels; a.n_classes = n_classes; a.ignore_label = ignore_label;
  a.lse = const_cast<float*>(lse); a.nll = const_cast<float*>(nll); a.stats = const_cast<double*>(stats); a.grad_out = grad_out; a.dlogits = dlogits; a.dld = dld;
  return csn_launch_ragged_seg_bwd(a, (hipStream_t)stream);
}

// ---- (13) fc_layer of the MinkowskiNet head: 1x1 convolution + BatchNorm + ReLU on point-major rows ----
static int rows_fc_dims(int n_rows, int c_in, int c_out) {
  if (n_rows <= 0) return CSN_E_ARG;
  if (c_in < 32 || c_in > 1024 || (c_in & 31) || !dim_ok(c_out)) return CSN_E_DIM;
  return 0;
}
static int rows_fc_pitch(long long ld, int width) {
  if (ld < width) return CSN_E_ARG;
  if (ld > (1 << 20)) return CSN_E_DIM;
  return (ld & 3) ? CSN_E_ALIGN : 0;
}

long long csn_rows_fc_workspace_bytes(int n_rows, int c_in, int c_out, int training, int backward) {
  if (rows_fc_dims(n_rows, c_in, c_out)) return 0;
  return csn_rows_fc_ws_bytes(n_rows, c_in, c_out, training != 0, backward != 0);
}

int csn_rows_fc_fwd_f32(const float* x, long long ld_x, int n_rows, int c_in, int c_out, const float* w, const float* bias,
                        const float* gamma, const float* beta, float* running_mean, float* running_var, float eps, float momentum,
                        int training, float* y, long long ld_y, float* z, long long ld_z, float* mean, float* invstd, void* ws,
                        long long ws_bytes, void* stream) {
  if (!x || !w || !gamma || !beta || !y) return CSN_E_ARG;
  if (training ? (!z || !mean || !invstd || !ws) : (!running_mean || !running_var)) return CSN_E_ARG;
  if (const int e = rows_fc_dims(n_rows, c_in, c_out)) return e;
  if (const int e = rows_fc_pitch(ld_x, c_in)) return e;
  if (const int e = rows_fc_pitch(ld_y, c_out)) return e;
  if (training) if (const int e = rows_fc_pitch(ld_z, c_out)) return e;
  if (mis16(x) || mis16(w) || mis16(y) || (training && (mis16(z) || mis16(ws)))) return CSN_E_PTR;
  if (training && n_rows == 1) return CSN_E_ARG;                  // a one-row batch has no variance (torch refuses it too)
  if (ws_bytes < csn_rows_fc_ws_bytes(n_rows, c_in, c_out, training != 0, 0)) return CSN_E_WORKSPACE;
  CsnRowsFcArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.w = w; a.bias = bias; a.gamma = gamma; a.beta = beta; a.running_mean = running_mean;
  a.running_var = running_var; a.eps = eps; a.momentum = momentum; a.training = training != 0; a.n_rows = n_rows; a.c_in = c_in;
  a.c_out = c_out; a.y = y; a.ld_y = (int)ld_y; a.z = z; a.ld_z = (int)ld_z; a.mean = mean; a.invstd = invstd; a.ws = ws;
  return csn_launch_rows_fc_fwd(a, rows_mode(), (hipStream_t)stream);
}

int csn_rows_fc_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const float* z, long long ld_z,
                        const float* x, long long ld_x, int n_rows, int c_in, int c_out, const float* w, const float* bias,
                        const float* gamma, const float* stat_mean, const float* stat_scale, float eps, int training, float* dx,
                        long long ld_dx, float* dw, float* dbias, float* dgamma, float* dbeta, void* ws, long long ws_bytes,
                        void* stream) {
  if (!dy || !y || !x || !w || !gamma || !stat_mean || !stat_scale || !dgamma || !dbeta || !ws) return CSN_E_ARG;
  if (training && !z) return CSN_E_ARG;
  if (rows_mode() == 3) return CSN_E_ARG;                         // fp16 single product: forward only — run the backward in mode 2
  if (const int e = rows_fc_dims(n_rows, c_in, c_out)) return e;
  if (const int e = rows_fc_pitch(ld_dy, c_out)) return e;
  if (const int e = rows_fc_pitch(ld_y, c_out)) return e;
  if (const int e = rows_fc_pitch(ld_x, c_in)) return e;
  if (training) if (const int e = rows_fc_pitch(ld_z, c_out)) return e;
  if (dx) if (const int e = rows_fc_pitch(ld_dx, c_in)) return e;
  if (mis16(dy) || mis16(y) || mis16(x) || mis16(w) || mis16(ws) || (training && mis16(z)) || (dx && mis16(dx)) || (dw && mis16(dw)))
    return CSN_E_PTR;
  if (training && n_rows == 1) return CSN_E_ARG;
  if (ws_bytes < csn_rows_fc_ws_bytes(n_rows, c_in, c_out, training != 0, 1)) return CSN_E_WORKSPACE;
  CsnRowsFcArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.w = w; a.bias = bias; a.gamma = gamma; a.eps = eps; a.training = training != 0; a.n_rows = n_rows;
  a.c_in = c_in; a.c_out = c_out; a.y = const_cast<float*>(y); a.ld_y = (int)ld_y; a.z = const_cast<float*>(z); a.ld_z = (int)ld_z;
  a.mean = const_cast<float*>(stat_mean); a.invstd = const_cast<float*>(stat_scale); a.dy = dy; a.ld_dy = (int)ld_dy; a.dx = dx;
  a.ld_dx = (int)ld_dx; a.dw = dw; a.dbias = dbias; a.dgamma = dgamma; a.dbeta = dbeta; a.ws = ws;
  return csn_launch_rows_fc_bwd(a, rows_mode(), (hipStream_t)stream);
}

// ---- (14) sparse 3D convolution on voxel rows over a kernel map ----
static int sparse_conv_dims(int n_in, int n_out, int kv, int c_in, int c_out) {
  if (n_in <= 0 || n_out <= 0) return CSN_E_ARG;
  if (kv != 1 && kv != 27 && kv != 125) return CSN_E_DIM;
  if (c_in < 32 || c_in > 256 || (c_in & 31) || c_out < 32 || c_out > 256 || (c_out & 31)) return CSN_E_DIM;
  return 0;
}
// (21) the sizes of an octant convolution (the two row counts in either order)
static int octant_dims(int n_fine, int n_coarse, int c_in, int c_out) {
  if (n_fine <= 0 || n_coarse <= 0) return CSN_E_ARG;
  if (c_in < 32 || c_in > 256 || (c_in & 31) || c_out < 32 || c_out > 256 || (c_out & 31)) return CSN_E_DIM;
  return 0;
}
// a row-major map of n rows: pitch % 4, >= its width, and the whole map inside one 2 GiB buffer window
static int sparse_conv_map(long long ld, int width, int n) {
  if (ld < width) return CSN_E_ARG;
  if (ld & 3) return CSN_E_ALIGN;
  if (ld > (1 << 20) || (long long)n * ld * 4 > 0x7fffffffLL) return CSN_E_DIM;
  return 0;
}
// a 16-bit row-major map of n rows (sections 24, 25, 28): pitch % 8, >= its width, and the whole map inside one 2 GiB buffer window
static int sparse_conv_map16(long long ld, int width, int n) {
  if (ld < width) return CSN_E_ARG;
  if (ld & 7) return CSN_E_ALIGN;
  if (ld > (1 << 20) || (long long)n * ld * 2 > 0x7fffffffLL) return CSN_E_DIM;
  return 0;
}
// a map beside its type flag: fp32 rows (0) or 16-bit rows (1), each by its own rule
static int map_of(int is16, long long ld, int width, int n) { return is16 ? sparse_conv_map16(ld, width, n) : sparse_conv_map(ld, width, n); }
static bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

long long csn_sparse_conv_workspace_bytes(int n_in, int n_out, int kv, int c_in, int c_out, int backward) {
  if (sparse_conv_dims(n_in, n_out, kv, c_in, c_out)) return 0;
  return csn_sparse_conv_ws_bytes(n_in, n_out, kv, c_in, c_out, backward != 0);
}

int csn_sparse_conv_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in, int c_out,
                            const float* w, const float* bias, float* y, long long ld_y, void* stream) {
  if (!x || !table || !w || !y) return CSN_E_ARG;
  if (const int e = sparse_conv_dims(n_in, n_out, kv, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_x, c_in, n_in)) return e;
  if (const int e = sparse_conv_map(ld_y, c_out, n_out)) return e;
  if (mis16(x) || mis16(w) || mis16(y) || off4(table)) return CSN_E_PTR;
  CsnSparseConvArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.n_in = n_in; a.fwd_table = table; a.n_out = n_out; a.kv = kv; a.c_in = c_in; a.c_out = c_out;
  a.w = w; a.bias = bias; a.y = y; a.ld_y = (int)ld_y;
  return csn_launch_sparse_conv_fwd(a, rows_mode(), (hipStream_t)stream);
}

int csn_sparse_conv_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_in, int n_out, int kv, int c_in,
                            int c_out, const int* fwd_table, const int* bwd_table, const float* w, float* dx, long long ld_dx,
                            float* dw, float* dbias, void* ws, long long ws_bytes, void* stream) {
  if (!dy || !ws) return CSN_E_ARG;
  if (dx && !w) return CSN_E_ARG;
  if (rows_mode() == 3) return CSN_E_ARG;                         // fp16 single product: forward only — run the backward in mode 2
  if (dx && !bwd_table && (!fwd_table || n_in != n_out)) return CSN_E_ARG;   // NULL: the stride-1 identity on fwd_table
  if (dw && (!fwd_table || !x)) return CSN_E_ARG;
  if (const int e = sparse_conv_dims(n_in, n_out, kv, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_dy, c_out, n_out)) return e;
  if (dw) if (const int e = sparse_conv_map(ld_x, c_in, n_in)) return e;
  if (dx) if (const int e = sparse_conv_map(ld_dx, c_in, n_in)) return e;
  if (mis16(dy) || mis16(ws) || (dx && (mis16(dx) || mis16(w))) || (dw && (mis16(dw) || mis16(x)))) return CSN_E_PTR;
  if (off4(fwd_table) || off4(bwd_table)) return CSN_E_PTR;
  if (ws_bytes < csn_sparse_conv_ws_bytes(n_in, n_out, kv, c_in, c_out, 1)) return CSN_E_WORKSPACE;
  CsnSparseConvArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.n_in = n_in; a.fwd_table = fwd_table; a.bwd_table = bwd_table; a.n_out = n_out; a.kv = kv;
  a.c_in = c_in; a.c_out = c_out; a.w = w; a.dy = dy; a.ld_dy = (int)ld_dy; a.dx = dx; a.ld_dx = (int)ld_dx; a.dw = dw; a.dbias = dbias;
  a.ws = ws;
  return csn_launch_sparse_conv_bwd(a, rows_mode(), (hipStream_t)stream);
}

// ---- (15) the HRNet backbone's fused tail ----
long long csn_sparse_conv_stats_workspace_bytes(int n_out, int c_out) {
  if (n_out <= 0 || c_out < 32 || c_out > 256 || (c_out & 31)) return 0;
  return csn_sparse_conv_stats_ws_bytes(n_out, c_out);
}

// (15) the whole map is one BatchNorm batch, (20) the batch per row group: one implementation each, `grouped` is the entry point
static int groups_args(const int* group_rows, int n_groups) {
  if (!group_rows || n_groups < 1) return CSN_E_ARG;
  if (n_groups > 8) return CSN_E_DIM;
  if (off4(group_rows)) return CSN_E_PTR;
  return 0;
}

// x16 (section 28, never with groups): x is bf16 rows, gathered as they lie by a launcher of their own
static int sparse_conv_stats_fwd_impl(const void* x, int x16, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                      int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd, float* running_mean,
                                      float* running_var, float eps, float momentum, bool grouped, const int* group_rows, int n_groups,
                                      void* ws, long long ws_bytes, void* stream) {
  if (!x || !table || !w || !z || !mean || !invstd || !ws) return CSN_E_ARG;
  if (grouped) if (const int e = groups_args(group_rows, n_groups)) return e;
  if (const int e = sparse_conv_dims(n_in, n_out, kv, c_in, c_out)) return e;
  if (const int e = map_of(x16, ld_x, c_in, n_in)) return e;
  if (const int e = sparse_conv_map(ld_z, c_out, n_out)) return e;
  if (mis16(x) || mis16(w) || mis16(z) || mis16(ws) || off4(table)) return CSN_E_PTR;
  if (n_out < 2 * (grouped ? n_groups : 1)) return CSN_E_ARG;    // every batch needs two rows: a one-row batch has no variance
  if (ws_bytes < csn_sparse_conv_stats_ws_bytes(n_out, c_out)) return CSN_E_WORKSPACE;
  CsnSparseConvArgs a{};
  a.x = static_cast<const float*>(x); a.ld_x = (int)ld_x; a.n_in = n_in; a.fwd_table = table; a.n_out = n_out; a.kv = kv; a.c_in = c_in;
  a.c_out = c_out; a.w = w; a.y = z; a.ld_y = (int)ld_z; a.ws = ws;
  if (x16) return csn_launch_sparse_conv_stats_fwd_x16(a, mean, invstd, running_mean, running_var, eps, momentum, (hipStream_t)stream);
  return csn_launch_sparse_conv_stats_fwd(a, grouped ? group_rows : nullptr, n_groups, mean, invstd, running_mean, running_var, eps,
                                          momentum, rows_mode(), (hipStream_t)stream);
}

int csn_sparse_conv_stats_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                  int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                  float* running_mean, float* running_var, float eps, float momentum, void* ws, long long ws_bytes,
                                  void* stream) {
  return sparse_conv_stats_fwd_impl(x, 0, ld_x, n_in, table, n_out, kv, c_in, c_out, w, z, ld_z, mean, invstd, running_mean, running_var,
                                    eps, momentum, false, nullptr, 0, ws, ws_bytes, stream);
}

static int bn_act_dims(int n_terms, int n_rows, int channels) {
  if (n_terms < 1 || n_terms > 3 || n_rows <= 0) return CSN_E_ARG;
  if (channels < 32 || channels > 256 || (channels & 31)) return CSN_E_DIM;
  return 0;
}

long long csn_rows_bn_act_workspace_bytes(int n_rows, int channels, int n_terms) {
  if (bn_act_dims(n_terms, n_rows, channels)) return 0;
  return csn_rows_bn_act_ws_bytes(n_rows, channels, n_terms, 1);
}

// the terms of CsnBnTerms, checked term by term and copied into `a`: the forward needs beta, the backward takes dz / dgamma / dbeta
static int bn_terms(CsnRowsBnActArgs& a, const CsnBnTerms* t, int n_terms, int n_rows, int channels, bool backward) {
  for (int m = 0; m < n_terms; ++m) {
    if (!t->z[m] || !t->mean[m] || !t->scale[m] || !t->gamma[m] || (!backward && !t->beta[m])) return CSN_E_ARG;
    if (const int e = sparse_conv_map(t->ld_z[m], channels, n_rows)) return e;
    if (backward && t->dz[m]) if (const int e = sparse_conv_map(t->ld_dz[m], channels, n_rows)) return e;
    if (mis16(t->z[m]) || (backward && t->dz[m] && mis16(t->dz[m]))) return CSN_E_PTR;
    a.z[m] = t->z[m]; a.ld_z[m] = (int)t->ld_z[m]; a.mean[m] = t->mean[m]; a.scale[m] = t->scale[m]; a.gamma[m] = t->gamma[m];
    if (!backward) { a.beta[m] = t->beta[m]; continue; }
    a.dz[m] = t->dz[m]; a.ld_dz[m] = (int)t->ld_dz[m]; a.dgamma[m] = t->dgamma[m]; a.dbeta[m] = t->dbeta[m];
  }
  return 0;
}

// r16 / y16: the type flags of r and y (1: bf16 rows); t16: the call of section 28, which has a launcher of its own whatever the flags say
static int rows_bn_act_fwd_impl(const CsnBnTerms* t, int n_terms, int n_rows, int channels, int training, float eps, bool grouped,
                                const int* group_rows, int n_groups, const void* r, int r16, long long ld_r, int relu, void* y, int y16,
                                long long ld_y, void* stream, bool t16 = false) {
  if (!t || !y) return CSN_E_ARG;
  if (grouped) if (const int e = groups_args(group_rows, n_groups)) return e;
  if (const int e = bn_act_dims(n_terms, n_rows, channels)) return e;
  CsnRowsBnActArgs a{};
  if (const int e = bn_terms(a, t, n_terms, n_rows, channels, false)) return e;
  if (const int e = map_of(y16, ld_y, channels, n_rows)) return e;
  if (r) if (const int e = map_of(r16, ld_r, channels, n_rows)) return e;
  if (mis16(y) || (r && mis16(r))) return CSN_E_PTR;
  a.n_terms = n_terms; a.n_rows = n_rows; a.C = channels; a.training = training != 0; a.relu = relu != 0; a.eps = eps;
  a.r = static_cast<const float*>(r); a.ld_r = (int)ld_r; a.y = static_cast<float*>(y); a.ld_y = (int)ld_y;
  if (t16) return csn_launch_rows_bn_act_fwd16(a, r16, y16, (hipStream_t)stream);
  return csn_launch_rows_bn_act_fwd(a, grouped ? group_rows : nullptr, n_groups, (hipStream_t)stream);
}

int csn_rows_bn_act_fwd_f32(const CsnBnTerms* t, int n_terms, int n_rows, int channels, int training, float eps, const float* r,
                            long long ld_r, int relu, float* y, long long ld_y, void* stream) {
  return rows_bn_act_fwd_impl(t, n_terms, n_rows, channels, training, eps, false, nullptr, 0, r, 0, ld_r, relu, y, 0, ld_y, stream);
}

// y16 (section 28, never with groups): y, the ReLU mask's operand, is bf16 rows, read by a launcher of their own
static int rows_bn_act_bwd_impl(const float* dy, long long ld_dy, const void* y, int y16, long long ld_y, const CsnBnTerms* t, int n_terms,
                                int n_rows, int channels, int training, float eps, bool grouped, const int* group_rows, int n_groups,
                                int relu, float* dr, long long ld_dr, void* ws, long long ws_bytes, void* stream) {
  if (!dy || !t || !ws || (relu && !y)) return CSN_E_ARG;
  if (grouped) if (const int e = groups_args(group_rows, n_groups)) return e;
  if (const int e = bn_act_dims(n_terms, n_rows, channels)) return e;
  CsnRowsBnActArgs a{};
  if (const int e = bn_terms(a, t, n_terms, n_rows, channels, true)) return e;
  if (const int e = sparse_conv_map(ld_dy, channels, n_rows)) return e;
  if (relu) if (const int e = map_of(y16, ld_y, channels, n_rows)) return e;
  if (dr) if (const int e = sparse_conv_map(ld_dr, channels, n_rows)) return e;
  if (mis16(dy) || mis16(ws) || (relu && mis16(y)) || (dr && mis16(dr))) return CSN_E_PTR;
  if (ws_bytes < csn_rows_bn_act_ws_bytes(n_rows, channels, n_terms, grouped ? n_groups : 1)) return CSN_E_WORKSPACE;
  a.n_terms = n_terms; a.n_rows = n_rows; a.C = channels; a.training = training != 0; a.relu = relu != 0; a.eps = eps;
  a.y = static_cast<float*>(const_cast<void*>(y)); a.ld_y = (int)ld_y; a.dy = dy; a.ld_dy = (int)ld_dy; a.dr = dr; a.ld_dr = (int)ld_dr;
  a.ws = ws;
  if (y16) return csn_launch_rows_bn_act_bwd16(a, (hipStream_t)stream);
  return csn_launch_rows_bn_act_bwd(a, grouped ? group_rows : nullptr, n_groups, (hipStream_t)stream);
}

int csn_rows_bn_act_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const CsnBnTerms* t, int n_terms,
                            int n_rows, int channels, int training, float eps, int relu, float* dr, long long ld_dr, void* ws,
                            long long ws_bytes, void* stream) {
  return rows_bn_act_bwd_impl(dy, ld_dy, y, 0, ld_y, t, n_terms, n_rows, channels, training, eps, false, nullptr, 0, relu, dr, ld_dr, ws,
                              ws_bytes, stream);
}

// ---- (19) the gather-GEMM with a BatchNorm + residual + ReLU epilogue (inference) ----
// What the "convolution + BatchNorm epilogue" calls check alike: (19) and (23) on fp32 maps (every flag 0), (24) and (25) on maps
// beside a type flag, behind the single-product gate (CONV_BN_M16).  CONV_BN_OCTANT: (21)'s sizes, kv is not read.  n_x: the rows of
// x, n_y: those of y and r, in either order where octant_dims wants (n_fine, n_coarse): it treats the two counts alike.  The caller
// refuses a NULL table before this and a misaligned one after it
enum { CONV_BN_M16 = 1, CONV_BN_OCTANT = 2 };
static int conv_bn_args(int form, const void* x, int x16, long long ld_x, int n_x, int n_y, int kv, int c_in, int c_out, const float* w,
                        const float* gamma, const float* beta, const float* running_mean, const float* running_var, const void* r, int r16,
                        long long ld_r, const void* y, int y16, long long ld_y) {
  if (!x || !w || !y || !gamma || !beta || !running_mean || !running_var) return CSN_E_ARG;
  if (form & CONV_BN_M16) {
    if ((x16 | r16 | y16) & ~1) return CSN_E_ARG;
    // single-product instances only: 16-bit maps under bf16x3 / fp32 would throw away what they pay for
    if (mode() < 2 || !t_rows16) return CSN_E_ARG;
  }
  if (const int e = (form & CONV_BN_OCTANT) ? octant_dims(n_x, n_y, c_in, c_out) : sparse_conv_dims(n_x, n_y, kv, c_in, c_out)) return e;
  if (const int e = map_of(x16, ld_x, c_in, n_x)) return e;
  if (const int e = map_of(y16, ld_y, c_out, n_y)) return e;
  if (r) if (const int e = map_of(r16, ld_r, c_out, n_y)) return e;
  if (r == y && (r16 != y16 || ld_r != ld_y)) return CSN_E_ARG;   // y as its own residual: element for element, or not at all
  if (mis16(x) || mis16(w) || mis16(y) || (r && mis16(r))) return CSN_E_PTR;
  return 0;
}
// the epilogue's vectors; the launches on 16-bit maps carry r in their own struct and pass none here
static CsnSconvBnArgs sconv_bn(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                               const float* r, long long ld_r, int relu) {
  CsnSconvBnArgs n{};
  n.gamma = gamma; n.beta = beta; n.running_mean = running_mean; n.running_var = running_var; n.eps = eps;
  n.r = r; n.ld_r = (int)ld_r; n.relu = relu != 0;
  return n;
}

int csn_sparse_conv_bn_act_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in, int c_out,
                                   const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const float* r, long long ld_r, int relu, float* y,
                                   long long ld_y, void* stream) {
  if (!table) return CSN_E_ARG;
  if (const int e = conv_bn_args(0, x, 0, ld_x, n_in, n_out, kv, c_in, c_out, w, gamma, beta, running_mean, running_var, r, 0, ld_r, y,
                                 0, ld_y)) return e;
  if (off4(table)) return CSN_E_PTR;
  CsnSparseConvArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.n_in = n_in; a.fwd_table = table; a.n_out = n_out; a.kv = kv; a.c_in = c_in; a.c_out = c_out;
  a.w = w; a.y = y; a.ld_y = (int)ld_y;
  return csn_launch_sparse_conv_bn_act_fwd(a, sconv_bn(gamma, beta, running_mean, running_var, eps, r, ld_r, relu), rows_mode(),
                                           (hipStream_t)stream);
}

// ---- (20) BatchNorm over row groups: the implementations of (15) with the batch per group, training mode ----
long long csn_sparse_conv_stats_groups_workspace_bytes(int n_out, int c_out, int n_groups) {
  if (n_groups < 1 || n_groups > 8) return 0;
  return csn_sparse_conv_stats_workspace_bytes(n_out, c_out);
}

int csn_sparse_conv_stats_groups_fwd_f32(const float* x, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                         int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                         float* running_mean, float* running_var, float eps, float momentum, const int* group_rows,
                                         int n_groups, void* ws, long long ws_bytes, void* stream) {
  return sparse_conv_stats_fwd_impl(x, 0, ld_x, n_in, table, n_out, kv, c_in, c_out, w, z, ld_z, mean, invstd, running_mean, running_var,
                                    eps, momentum, true, group_rows, n_groups, ws, ws_bytes, stream);
}

long long csn_rows_bn_act_groups_workspace_bytes(int n_rows, int channels, int n_terms, int n_groups) {
  if (bn_act_dims(n_terms, n_rows, channels) || n_groups < 1 || n_groups > 8) return 0;
  return csn_rows_bn_act_ws_bytes(n_rows, channels, n_terms, n_groups);
}

int csn_rows_bn_act_groups_fwd_f32(const CsnBnTerms* t, int n_terms, int n_rows, int channels, const int* group_rows, int n_groups,
                                   const float* r, long long ld_r, int relu, float* y, long long ld_y, void* stream) {
  return rows_bn_act_fwd_impl(t, n_terms, n_rows, channels, 1, 0.f, true, group_rows, n_groups, r, 0, ld_r, relu, y, 0, ld_y, stream);
}

int csn_rows_bn_act_groups_bwd_f32(const float* dy, long long ld_dy, const float* y, long long ld_y, const CsnBnTerms* t, int n_terms,
                                   int n_rows, int channels, const int* group_rows, int n_groups, int relu, float* dr, long long ld_dr,
                                   void* ws, long long ws_bytes, void* stream) {
  return rows_bn_act_bwd_impl(dy, ld_dy, y, 0, ld_y, t, n_terms, n_rows, channels, 1, 0.f, true, group_rows, n_groups, relu, dr, ld_dr, ws,
                              ws_bytes, stream);
}

// ---- (21) kernel-2 stride-2 convolution and its transposed form over an octant map ----
static int octant_mode() { return mode() != 0; }                 // no single-product instances: modes 2 / 3 run as bf16x3

long long csn_octant_conv_workspace_bytes(int n_fine, int n_coarse, int c_in, int c_out, int up, int backward) {
  if (octant_dims(n_fine, n_coarse, c_in, c_out)) return 0;
  return csn_octant_conv_ws_bytes(n_fine, n_coarse, c_in, c_out, up != 0, backward != 0);
}

// the struct of every octant launch but the 16-bit ones: down names children alone, up parent / order / seg (a backward: what it reads);
// y / ld_y are z's of the statistics forms; bias, y and ws NULL where the call has none
static CsnOctantConvArgs octant_args(const float* x, long long ld_x, int n_fine, int n_coarse, int c_in, int c_out, const int* children,
                                     const int* parent, const int* order, const int* seg, const float* w, const float* bias, float* y,
                                     long long ld_y, void* ws) {
  CsnOctantConvArgs a{};
  a.x = x; a.ld_x = (int)ld_x; a.n_fine = n_fine; a.n_coarse = n_coarse; a.c_in = c_in; a.c_out = c_out;
  a.children = children; a.parent = parent; a.order = order; a.seg = seg;
  a.w = w; a.bias = bias; a.y = y; a.ld_y = (int)ld_y; a.ws = ws;
  return a;
}

int csn_octant_down_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in, int c_out,
                            const float* w, const float* bias, float* y, long long ld_y, void* stream) {
  if (!x || !children || !w || !y) return CSN_E_ARG;
  if (const int e = octant_dims(n_fine, n_coarse, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_x, c_in, n_fine)) return e;
  if (const int e = sparse_conv_map(ld_y, c_out, n_coarse)) return e;
  if (mis16(x) || mis16(w) || mis16(y) || off4(children)) return CSN_E_PTR;
  return csn_launch_octant_down_fwd(octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, children, nullptr, nullptr, nullptr, w, bias, y,
                                                ld_y, nullptr), octant_mode(), (hipStream_t)stream);
}

int csn_octant_up_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order, const int* seg,
                          int n_fine, int c_in, int c_out, const float* w, const float* bias, float* y, long long ld_y,
                          void* stream) {
  if (!x || !parent || !order || !seg || !w || !y) return CSN_E_ARG;
  if (const int e = octant_dims(n_fine, n_coarse, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_x, c_in, n_coarse)) return e;
  if (const int e = sparse_conv_map(ld_y, c_out, n_fine)) return e;
  if (mis16(x) || mis16(w) || mis16(y) || off4(parent) || off4(order) || off4(seg)) return CSN_E_PTR;
  return csn_launch_octant_up_fwd(octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, nullptr, parent, order, seg, w, bias, y, ld_y,
                                              nullptr), octant_mode(), (hipStream_t)stream);
}

// the checks the two backward entry points share, and their struct: n_x / n_dy are the rows of x / dy, `one` says whether dx is the
// one-weight form
static int octant_bwd_args(CsnOctantConvArgs& a, const float* dy, long long ld_dy, const float* x, long long ld_x, int n_x, int n_dy,
                           int n_fine, int n_coarse, int c_in, int c_out, const int* children, const int* parent, const int* order,
                           const int* seg, const float* w, float* dx, long long ld_dx, float* dw, float* dbias, void* ws,
                           long long ws_bytes, bool one, bool up) {
  if (!dy || !ws) return CSN_E_ARG;
  if (dx && (!w || (one ? (!parent || !order || !seg) : !children))) return CSN_E_ARG;
  if (dw && (!x || !parent || !order || !seg)) return CSN_E_ARG;
  if (const int e = octant_dims(n_fine, n_coarse, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_dy, c_out, n_dy)) return e;
  if (dw) if (const int e = sparse_conv_map(ld_x, c_in, n_x)) return e;
  if (dx) if (const int e = sparse_conv_map(ld_dx, c_in, n_x)) return e;
  if (mis16(dy) || mis16(ws) || (dx && (mis16(dx) || mis16(w))) || (dw && (mis16(dw) || mis16(x)))) return CSN_E_PTR;
  if (off4(children) || off4(parent) || off4(order) || off4(seg)) return CSN_E_PTR;
  if (ws_bytes < csn_octant_conv_ws_bytes(n_fine, n_coarse, c_in, c_out, up, 1)) return CSN_E_WORKSPACE;
  a = octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, children, parent, order, seg, w, nullptr, nullptr, 0, ws);
  a.dy = dy; a.ld_dy = (int)ld_dy; a.dx = dx; a.ld_dx = (int)ld_dx; a.dw = dw; a.dbias = dbias;
  return 0;
}

int csn_octant_down_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_fine, int n_coarse, int c_in,
                            int c_out, const int* parent, const int* order, const int* seg, const float* w, float* dx,
                            long long ld_dx, float* dw, float* dbias, void* ws, long long ws_bytes, void* stream) {
  CsnOctantConvArgs a;
  if (const int e = octant_bwd_args(a, dy, ld_dy, x, ld_x, n_fine, n_coarse, n_fine, n_coarse, c_in, c_out, nullptr, parent, order, seg, w,
                                    dx, ld_dx, dw, dbias, ws, ws_bytes, true, false)) return e;
  return csn_launch_octant_down_bwd(a, octant_mode(), (hipStream_t)stream);
}

int csn_octant_up_bwd_f32(const float* dy, long long ld_dy, const float* x, long long ld_x, int n_fine, int n_coarse, int c_in,
                          int c_out, const int* children, const int* parent, const int* order, const int* seg, const float* w,
                          float* dx, long long ld_dx, float* dw, float* dbias, void* ws, long long ws_bytes, void* stream) {
  CsnOctantConvArgs a;
  if (const int e = octant_bwd_args(a, dy, ld_dy, x, ld_x, n_coarse, n_fine, n_fine, n_coarse, c_in, c_out, children, parent, order, seg, w,
                                    dx, ld_dx, dw, dbias, ws, ws_bytes, false, true)) return e;
  return csn_launch_octant_up_bwd(a, octant_mode(), (hipStream_t)stream);
}

// ---- (23) the octant convolutions with a BatchNorm + residual + ReLU epilogue (inference) ----
// (21)'s checks on the maps, (19)'s on the residual: conv_bn_args
int csn_octant_down_bn_act_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in, int c_out,
                                   const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const float* r, long long ld_r, int relu, float* y,
                                   long long ld_y, void* stream) {
  if (!children) return CSN_E_ARG;
  if (const int e = conv_bn_args(CONV_BN_OCTANT, x, 0, ld_x, n_fine, n_coarse, 0, c_in, c_out, w, gamma, beta, running_mean, running_var,
                                 r, 0, ld_r, y, 0, ld_y)) return e;
  if (off4(children)) return CSN_E_PTR;
  return csn_launch_octant_down_bn_act_fwd(octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, children, nullptr, nullptr, nullptr, w,
                                                       nullptr, y, ld_y, nullptr),
                                           sconv_bn(gamma, beta, running_mean, running_var, eps, r, ld_r, relu), octant_mode(),
                                           (hipStream_t)stream);
}

int csn_octant_up_bn_act_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order, const int* seg,
                                 int n_fine, int c_in, int c_out, const float* w, const float* gamma, const float* beta,
                                 const float* running_mean, const float* running_var, float eps, const float* r, long long ld_r,
                                 int relu, float* y, long long ld_y, void* stream) {
  if (!parent || !order || !seg) return CSN_E_ARG;
  if (const int e = conv_bn_args(CONV_BN_OCTANT, x, 0, ld_x, n_coarse, n_fine, 0, c_in, c_out, w, gamma, beta, running_mean, running_var,
                                 r, 0, ld_r, y, 0, ld_y)) return e;
  if (off4(parent) || off4(order) || off4(seg)) return CSN_E_PTR;
  return csn_launch_octant_up_bn_act_fwd(octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, nullptr, parent, order, seg, w, nullptr, y,
                                                     ld_y, nullptr),
                                         sconv_bn(gamma, beta, running_mean, running_var, eps, r, ld_r, relu), octant_mode(),
                                         (hipStream_t)stream);
}

// ---- (26) the octant convolutions with the BatchNorm statistics epilogue (training) ----
long long csn_octant_stats_workspace_bytes(int n_fine, int n_coarse, int c_out, int up) {
  if (octant_dims(n_fine, n_coarse, 32, c_out)) return 0;
  return csn_octant_stats_ws_bytes(n_fine, n_coarse, c_out, up != 0);
}

// (21)'s checks on the maps, (15a)'s on the batch and the workspace; n_x / n_z: the rows of x / z
static int octant_stats_args(long long ld_x, int n_x, int n_z, int n_fine, int n_coarse, int c_in, int c_out, long long ld_z,
                             long long ws_bytes, bool up) {
  if (const int e = octant_dims(n_fine, n_coarse, c_in, c_out)) return e;
  if (const int e = sparse_conv_map(ld_x, c_in, n_x)) return e;
  if (const int e = sparse_conv_map(ld_z, c_out, n_z)) return e;
  if (n_z < 2) return CSN_E_ARG;                                  // a one-row batch has no variance
  if (ws_bytes < csn_octant_stats_ws_bytes(n_fine, n_coarse, c_out, up)) return CSN_E_WORKSPACE;
  return 0;
}

int csn_octant_down_stats_fwd_f32(const float* x, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in, int c_out,
                                  const float* w, float* z, long long ld_z, float* mean, float* invstd, float* running_mean,
                                  float* running_var, float eps, float momentum, void* ws, long long ws_bytes, void* stream) {
  if (!x || !children || !w || !z || !mean || !invstd || !ws) return CSN_E_ARG;
  if (const int e = octant_stats_args(ld_x, n_fine, n_coarse, n_fine, n_coarse, c_in, c_out, ld_z, ws_bytes, false)) return e;
  if (mis16(x) || mis16(w) || mis16(z) || mis16(ws) || off4(children)) return CSN_E_PTR;
  const CsnOctantConvArgs a = octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, children, nullptr, nullptr, nullptr, w, nullptr, z,
                                          ld_z, ws);
  return csn_launch_octant_down_stats_fwd(a, mean, invstd, running_mean, running_var, eps, momentum, octant_mode(), (hipStream_t)stream);
}

int csn_octant_up_stats_fwd_f32(const float* x, long long ld_x, int n_coarse, const int* parent, const int* order, const int* seg,
                                int n_fine, int c_in, int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd,
                                float* running_mean, float* running_var, float eps, float momentum, void* ws, long long ws_bytes,
                                void* stream) {
  if (!x || !parent || !order || !seg || !w || !z || !mean || !invstd || !ws) return CSN_E_ARG;
  if (const int e = octant_stats_args(ld_x, n_coarse, n_fine, n_fine, n_coarse, c_in, c_out, ld_z, ws_bytes, true)) return e;
  if (mis16(x) || mis16(w) || mis16(z) || mis16(ws) || off4(parent) || off4(order) || off4(seg)) return CSN_E_PTR;
  const CsnOctantConvArgs a = octant_args(x, ld_x, n_fine, n_coarse, c_in, c_out, nullptr, parent, order, seg, w, nullptr, z, ld_z,
                                          ws);
  return csn_launch_octant_up_stats_fwd(a, mean, invstd, running_mean, running_var, eps, momentum, octant_mode(), (hipStream_t)stream);
}

// ---- (27) (15a) over a concatenation that is never formed ----
long long csn_sparse_conv_cat_stats_workspace_bytes(int n_out, int c_out) { return csn_sparse_conv_stats_workspace_bytes(n_out, c_out); }

int csn_sparse_conv_cat_stats_fwd_f32(const CsnCatParts* parts, int n_parts, int n_in, const int* table, int n_out, int kv, int c_out,
                                      const float* w, float* z, long long ld_z, float* mean, float* invstd, float* running_mean,
                                      float* running_var, float eps, float momentum, void* ws, long long ws_bytes, void* stream) {
  if (!parts || n_parts < 1 || n_parts > 4 || !table || !w || !z || !mean || !invstd || !ws) return CSN_E_ARG;
  if (kv != 1 && kv != 27) return CSN_E_DIM;
  const float* x[4]; int ld_x[4], c_in[4];
  long long sum = 0;
  for (int m = 0; m < n_parts; ++m) {
    if (!parts->x[m]) return CSN_E_ARG;
    if (const int e = sparse_conv_dims(n_in, n_out, kv, parts->c_in[m], c_out)) return e;
    if (const int e = sparse_conv_map(parts->ld_x[m], parts->c_in[m], n_in)) return e;
    if (mis16(parts->x[m])) return CSN_E_PTR;
    x[m] = parts->x[m]; ld_x[m] = (int)parts->ld_x[m]; c_in[m] = parts->c_in[m];
    sum += c_in[m];
  }
  if (const int e = sparse_conv_map(ld_z, c_out, n_out)) return e;
  if (mis16(w) || mis16(z) || mis16(ws) || off4(table)) return CSN_E_PTR;
  if (n_out < 2) return CSN_E_ARG;                                // a one-row batch has no variance
  if (ws_bytes < csn_sparse_conv_stats_ws_bytes(n_out, c_out)) return CSN_E_WORKSPACE;
  CsnSparseConvArgs a{};
  a.n_in = n_in; a.fwd_table = table; a.n_out = n_out; a.kv = kv; a.c_in = (int)sum; a.c_out = c_out; a.w = w; a.y = z; a.ld_y = (int)ld_z;
  a.ws = ws;
  return csn_launch_sparse_conv_cat_stats_fwd(a, x, ld_x, c_in, n_parts, mean, invstd, running_mean, running_var, eps, momentum,
                                              rows_mode(), (hipStream_t)stream);
}

// ---- (24) the launch of (19) on 16-bit maps: x, r and y each fp32 rows or rows of the math mode's 16-bit type ----
int csn_sparse_conv_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                   int c_out, const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const void* r, int r16, long long ld_r, int relu, void* y,
                                   int y16, long long ld_y, void* stream) {
  if (!table) return CSN_E_ARG;
  if (const int e = conv_bn_args(CONV_BN_M16, x, x16, ld_x, n_in, n_out, kv, c_in, c_out, w, gamma, beta, running_mean, running_var, r,
                                 r16, ld_r, y, y16, ld_y)) return e;
  if (off4(table)) return CSN_E_PTR;
  CsnSparseConvM16Args a{};
  a.x = x; a.x16 = x16; a.ld_x = (int)ld_x; a.n_in = n_in; a.table = table; a.n_out = n_out; a.kv = kv; a.c_in = c_in; a.c_out = c_out;
  a.w = w; a.r = r; a.r16 = r16; a.ld_r = (int)ld_r; a.y = y; a.y16 = y16; a.ld_y = (int)ld_y;
  return csn_launch_sparse_conv_bn_act_fwd_m16(a, sconv_bn(gamma, beta, running_mean, running_var, eps, nullptr, 0, relu), mode(),
                                               (hipStream_t)stream);
}

// ---- (28) training on bf16 activation maps: (15a), (15b) and (14)'s backward with a type flag beside the map that may be bf16 ----
// math mode 2 behind csn_set_thread_rows16, and nothing else: there alone the fp32 form rounds these maps to bf16 itself
static int train16_mode(int flags) {
  if (flags & ~1) return CSN_E_ARG;
  return mode() == 2 && t_rows16 ? 0 : CSN_E_ARG;
}

int csn_sparse_conv_stats_fwd_t16(const void* x, int x16, long long ld_x, int n_in, const int* table, int n_out, int kv, int c_in,
                                  int c_out, const float* w, float* z, long long ld_z, float* mean, float* invstd, float* running_mean,
                                  float* running_var, float eps, float momentum, void* ws, long long ws_bytes, void* stream) {
  if (const int e = train16_mode(x16)) return e;
  return sparse_conv_stats_fwd_impl(x, x16, ld_x, n_in, table, n_out, kv, c_in, c_out, w, z, ld_z, mean, invstd, running_mean, running_var,
                                    eps, momentum, false, nullptr, 0, ws, ws_bytes, stream);
}

int csn_rows_bn_act_fwd_t16(const CsnBnTerms* t, int n_terms, int n_rows, int channels, int training, float eps, const void* r, int r16,
                            long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream) {
  if (const int e = train16_mode(r16 | y16)) return e;
  return rows_bn_act_fwd_impl(t, n_terms, n_rows, channels, training, eps, false, nullptr, 0, r, r16, ld_r, relu, y, y16, ld_y, stream,
                              /*t16=*/true);
}

int csn_rows_bn_act_bwd_t16(const float* dy, long long ld_dy, const void* y, int y16, long long ld_y, const CsnBnTerms* t, int n_terms,
                            int n_rows, int channels, int training, float eps, int relu, float* dr, long long ld_dr, void* ws,
                            long long ws_bytes, void* stream) {
  if (const int e = train16_mode(y16)) return e;
  // the mask is the only use of y: without it the pointer is dropped and (15b) itself runs
  return rows_bn_act_bwd_impl(dy, ld_dy, relu ? y : nullptr, relu ? y16 : 0, ld_y, t, n_terms, n_rows, channels, training, eps, false,
                              nullptr, 0, relu, dr, ld_dr, ws, ws_bytes, stream);
}

int csn_sparse_conv_bwd_t16(const float* dy, long long ld_dy, const void* x, int x16, long long ld_x, int n_in, int n_out, int kv,
                            int c_in, int c_out, const int* fwd_table, const int* bwd_table, const float* w, float* dx, long long ld_dx,
                            float* dw, float* dbias, void* ws, long long ws_bytes, void* stream) {
  if (const int e = train16_mode(x16)) return e;
  if (!x16 || !dw)                                                // x is the weight gradient's operand alone
    return csn_sparse_conv_bwd_f32(dy, ld_dy, dw ? static_cast<const float*>(x) : nullptr, ld_x, n_in, n_out, kv, c_in, c_out, fwd_table,
                                   bwd_table, w, dx, ld_dx, dw, dbias, ws, ws_bytes, stream);
  if (!dy || !ws || !fwd_table || !x) return CSN_E_ARG;
  if (const int e = sparse_conv_dims(n_in, n_out, kv, c_in, c_out)) return e;
  if (const int e = sparse_conv_map16(ld_x, c_in, n_in)) return e;
  if (mis16(x) || mis16(dw)) return CSN_E_PTR;
  // dx and dbias: (14)'s backward as it is (it checks dy, the tables, w, dx, ws and the workspace size for all three outputs)
  if (const int e = csn_sparse_conv_bwd_f32(dy, ld_dy, nullptr, 0, n_in, n_out, kv, c_in, c_out, fwd_table, bwd_table, w, dx, ld_dx, nullptr,
                                            dbias, ws, ws_bytes, stream))
    return e;
  CsnSparseConvArgs a{};
  a.x = static_cast<const float*>(x); a.ld_x = (int)ld_x; a.n_in = n_in; a.fwd_table = fwd_table; a.n_out = n_out; a.kv = kv;
  a.c_in = c_in; a.c_out = c_out; a.dy = dy; a.ld_dy = (int)ld_dy; a.dw = dw; a.ws = ws;
  return csn_launch_sparse_conv_wgrad_x16(a, (hipStream_t)stream);
}

// ---- (25) the launches of (23) as one 16-bit product on maps that are each fp32 rows or rows of the mode's 16-bit type ----
// (24)'s mode and flag checks, (21)'s on the sizes, each map by its own type's rule: conv_bn_args
static CsnOctantM16Args octant_m16(const void* x, int x16, long long ld_x, int n_fine, int n_coarse, int c_in, int c_out,
                                   const int* children, const int* parent, const int* order, const int* seg, const float* w, const void* r,
                                   int r16, long long ld_r, void* y, int y16, long long ld_y) {
  CsnOctantM16Args a{};
  a.x = x; a.x16 = x16; a.ld_x = (int)ld_x; a.n_fine = n_fine; a.n_coarse = n_coarse; a.c_in = c_in; a.c_out = c_out;
  a.children = children; a.parent = parent; a.order = order; a.seg = seg;
  a.w = w; a.r = r; a.r16 = r16; a.ld_r = (int)ld_r; a.y = y; a.y16 = y16; a.ld_y = (int)ld_y;
  return a;
}

int csn_octant_down_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_fine, const int* children, int n_coarse, int c_in,
                                   int c_out, const float* w, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, const void* r, int r16, long long ld_r, int relu, void* y,
                                   int y16, long long ld_y, void* stream) {
  if (!children) return CSN_E_ARG;
  if (const int e = conv_bn_args(CONV_BN_M16 | CONV_BN_OCTANT, x, x16, ld_x, n_fine, n_coarse, 0, c_in, c_out, w, gamma, beta, running_mean,
                                 running_var, r, r16, ld_r, y, y16, ld_y)) return e;
  if (off4(children)) return CSN_E_PTR;
  return csn_launch_octant_down_bn_act_fwd_m16(octant_m16(x, x16, ld_x, n_fine, n_coarse, c_in, c_out, children, nullptr, nullptr, nullptr,
                                                          w, r, r16, ld_r, y, y16, ld_y),
                                               sconv_bn(gamma, beta, running_mean, running_var, eps, nullptr, 0, relu), mode(),
                                               (hipStream_t)stream);
}

int csn_octant_up_bn_act_fwd_m16(const void* x, int x16, long long ld_x, int n_coarse, const int* parent, const int* order,
                                 const int* seg, int n_fine, int c_in, int c_out, const float* w, const float* gamma,
                                 const float* beta, const float* running_mean, const float* running_var, float eps, const void* r,
                                 int r16, long long ld_r, int relu, void* y, int y16, long long ld_y, void* stream) {
  if (!parent || !order || !seg) return CSN_E_ARG;
  if (const int e = conv_bn_args(CONV_BN_M16 | CONV_BN_OCTANT, x, x16, ld_x, n_coarse, n_fine, 0, c_in, c_out, w, gamma, beta, running_mean,
                                 running_var, r, r16, ld_r, y, y16, ld_y)) return e;
  if (off4(parent) || off4(order) || off4(seg)) return CSN_E_PTR;
  return csn_launch_octant_up_bn_act_fwd_m16(octant_m16(x, x16, ld_x, n_fine, n_coarse, c_in, c_out, nullptr, parent, order, seg, w, r, r16,
                                                        ld_r, y, y16, ld_y),
                                             sconv_bn(gamma, beta, running_mean, running_var, eps, nullptr, 0, relu), mode(),
                                             (hipStream_t)stream);
}

// ---- (16) point fields: voxel means, interpolation onto points and its adjoint ----
static bool mis4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

int csn_voxel_mean_f32(const float* feats, long long ld_feats, int n_points, const int* vox_ptr, const int* vox_pts, int n_voxels,
                       int channels, float* out, long long ld_out, void* stream) {
  if (!feats || !vox_ptr || !vox_pts || !out) return CSN_E_ARG;
  if (n_points < 1 || n_voxels < 1 || n_voxels > n_points) return CSN_E_ARG;
  if (channels < 1 || channels > 64) return CSN_E_DIM;
  if (ld_feats < channels || ld_out < channels) return CSN_E_ARG;
  if (mis4(feats) || mis4(out) || mis4(vox_ptr) || mis4(vox_pts)) return CSN_E_PTR;
  CsnPointFieldArgs a{};
  a.dy = feats; a.ld_dy = ld_feats; a.n_points = n_points; a.vox_ptr = vox_ptr; a.vox_pts = vox_pts; a.n_voxels = n_voxels;
  a.C = channels; a.dz = out; a.ld_dz = ld_out;
  return csn_launch_voxel_mean(a, (hipStream_t)stream);
}

int csn_point_interp_fwd_f32(const float* z, long long ld_z, int n_voxels, const float* coords, const int* home, const int* table,
                             int n_points, int channels, float* y, long long ld_y, void* stream) {
  if (!z || !coords || !home || !table || !y) return CSN_E_ARG;
  if (n_points < 1 || n_voxels < 1) return CSN_E_ARG;
  if (channels < 1 || channels > 1024) return CSN_E_DIM;
  if (ld_z < channels || ld_y < channels) return CSN_E_ARG;
  if (mis16(coords) || mis4(z) || mis4(y) || mis4(home) || mis4(table)) return CSN_E_PTR;
  CsnPointFieldArgs a{};
  a.z = z; a.ld_z = ld_z; a.n_voxels = n_voxels; a.coords = coords; a.home = home; a.table = table; a.n_points = n_points;
  a.C = channels; a.y = y; a.ld_y = ld_y;
  return csn_launch_point_interp_fwd(a, (hipStream_t)stream);
}

int csn_point_interp_bwd_f32(const float* dy, long long ld_dy, int n_points, const float* coords, const int* vox_ptr,
                             const int* vox_pts, const int* table, int n_voxels, int channels, float* dz, long long ld_dz,
                             void* stream) {
  if (!dy || !coords || !vox_ptr || !vox_pts || !table || !dz) return CSN_E_ARG;
  if (n_points < 1 || n_voxels < 1) return CSN_E_ARG;
  if (channels < 1 || channels > 1024) return CSN_E_DIM;
  if (ld_dy < channels || ld_dz < channels) return CSN_E_ARG;
  if (mis16(coords) || mis4(dy) || mis4(dz) || mis4(vox_ptr) || mis4(vox_pts) || mis4(table)) return CSN_E_PTR;
  CsnPointFieldArgs a{};
  a.dy = dy; a.ld_dy = ld_dy; a.n_points = n_points; a.coords = coords; a.vox_ptr = vox_ptr; a.vox_pts = vox_pts; a.table = table;
  a.n_voxels = n_voxels; a.C = channels; a.dz = dz; a.ld_dz = ld_dz;
  return csn_launch_point_interp_bwd(a, (hipStream_t)stream);
}

// ---- (17) kernel maps: packed keys, the coarser level's keys, the offset tables ----
static bool mis8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }

int csn_coord_keys_i64(const long long* coords, int n, int tensor_stride, long long* keys, int* status, void* stream) {
  if (!coords || !keys || !status) return CSN_E_ARG;
  if (n < 1 || tensor_stride < 1) return CSN_E_ARG;
  if (mis8(coords) || mis8(keys) || mis4(status)) return CSN_E_PTR;
  return csn_launch_coord_keys(coords, n, tensor_stride, keys, status, (hipStream_t)stream);
}

int csn_coord_down_i64(const long long* keys, int n, int out_tensor_stride, long long* down_keys, void* stream) {
  if (!keys || !down_keys) return CSN_E_ARG;
  if (n < 1 || out_tensor_stride < 1) return CSN_E_ARG;
  if (mis8(keys) || mis8(down_keys)) return CSN_E_PTR;
  return csn_launch_coord_down(keys, n, out_tensor_stride, down_keys, (hipStream_t)stream);
}

int csn_kernel_map_i32(const long long* set_keys, const int* set_rows, int n_set, const long long* query_keys, int n_query,
                       int kernel_size, int step, int* table, int* status, void* stream) {
  if (!set_keys || !query_keys || !table || !status) return CSN_E_ARG;
  if (n_set < 1 || n_query < 1 || step == 0) return CSN_E_ARG;
  if (kernel_size != 1 && kernel_size != 3 && kernel_size != 5) return CSN_E_DIM;
  if (mis8(set_keys) || mis8(query_keys) || mis4(table) || mis4(status) || (set_rows && mis4(set_rows))) return CSN_E_PTR;
  CsnKernelMapArgs a{};
  a.set_keys = set_keys; a.set_rows = set_rows; a.n_set = n_set; a.query_keys = query_keys; a.n_query = n_query;
  a.kernel_size = kernel_size; a.step = step; a.table = table; a.status = status;
  return csn_launch_kernel_map(a, (hipStream_t)stream);
}

// ---- (22) octant maps: the partition of a fine set by its coarse set, the rows sorted by octant ----
int csn_octant_partition_i32(const long long* fine_keys, const long long* fine_sorted, int n_fine, int tensor_stride,
                             const long long* coarse_keys, const int* coarse_rows, int n_coarse, int* parent, int* octant, int* children,
                             int* status, void* stream) {
  if (!fine_keys || !coarse_keys || !parent || !octant || !children || !status) return CSN_E_ARG;
  if (n_fine < 1 || n_coarse < 1 || tensor_stride < 1) return CSN_E_ARG;
  if (mis8(fine_keys) || mis8(coarse_keys) || (fine_sorted && mis8(fine_sorted)) || (coarse_rows && mis4(coarse_rows))) return CSN_E_PTR;
  if (mis4(parent) || mis4(octant) || mis4(children) || mis4(status)) return CSN_E_PTR;
  CsnOctantMapArgs a{};
  a.fine_keys = fine_keys; a.fine_sorted = fine_sorted; a.n_fine = n_fine; a.tensor_stride = tensor_stride; a.coarse_keys = coarse_keys;
  a.coarse_rows = coarse_rows; a.n_coarse = n_coarse; a.parent = parent; a.octant = octant; a.children = children; a.status = status;
  return csn_launch_octant_partition(a, (hipStream_t)stream);
}

long long csn_octant_order_workspace_bytes(int n) {
  if (n < 1) return 0;
  return 8 * csn_octant_order_tiles(n) * (long long)sizeof(int);
}

int csn_octant_order_i32(const int* octant, int n, int* order, int* seg, void* ws, long long ws_bytes, int* status, void* stream) {
  if (!octant || !order || !seg || !ws || !status) return CSN_E_ARG;
  if (n < 1) return CSN_E_ARG;
  if (mis4(octant) || mis4(order) || mis4(seg) || mis4(ws) || mis4(status)) return CSN_E_PTR;
  if (ws_bytes < csn_octant_order_workspace_bytes(n)) return CSN_E_WORKSPACE;
  return csn_launch_octant_order(octant, n, order, seg, static_cast<int*>(ws), status, (hipStream_t)stream);
}

// ---- (18) resident point collections: normalise, bound, augment + collate + key; a PointField's index arrays ----
static int points_collection(const float* points, const long long* offsets, int n_shapes, long long n_total, const int* status) {
  if (!points || !offsets || !status) return CSN_E_ARG;
  if (n_shapes < 1 || n_total < 1) return CSN_E_ARG;
  if (mis4(points) || mis8(offsets) || mis4(status)) return CSN_E_PTR;
  return 0;
}

int csn_points_normalize_f32(const float* points, const long long* offsets, int n_shapes, long long n_total, int method, float* out,
                             int* status, void* stream) {
  if (const int e = points_collection(points, offsets, n_shapes, n_total, status)) return e;
  if (!out || (method != 0 && method != 1)) return CSN_E_ARG;
  if (mis4(out)) return CSN_E_PTR;
  CsnPointsArgs a{};
  a.points = points; a.offsets = offsets; a.n_shapes = n_shapes; a.n_total = n_total; a.method = method; a.out = out; a.status = status;
  return csn_launch_points_normalize(a, (hipStream_t)stream);
}

int csn_points_bounds_f64(const float* points, const long long* offsets, int n_shapes, long long n_total, const long long* idx,
                          const double* params, int n_items, double* bounds, int* status, void* stream) {
  if (const int e = points_collection(points, offsets, n_shapes, n_total, status)) return e;
  if (!idx || !params || !bounds || n_items < 1) return CSN_E_ARG;
  if (mis8(idx) || mis8(params) || mis8(bounds)) return CSN_E_PTR;
  CsnPointsArgs a{};
  a.points = points; a.offsets = offsets; a.n_shapes = n_shapes; a.n_total = n_total; a.idx = idx; a.params = params;
  a.n_items = n_items; a.bounds = bounds; a.status = status;
  return csn_launch_points_bounds(a, (hipStream_t)stream);
}

int csn_points_batch_f32(const float* points, const int* labels, const long long* offsets, int n_shapes, long long n_total,
                         const long long* idx, const long long* out_offsets, const double* params, const double* bounds, int n_items,
                         int max_points, double sigma, double clip, double voxel_size, float* coords, float* feats, long long* labels_out,
                         long long* keys, long long n_out, int* status, void* stream) {
  if (const int e = points_collection(points, offsets, n_shapes, n_total, status)) return e;
  if (!idx || !out_offsets || !params || !bounds || !coords || !feats || !keys || (labels && !labels_out)) return CSN_E_ARG;
  if (n_items < 1 || max_points < 1 || n_out < 1) return CSN_E_ARG;
  if (!(sigma >= 0.0) || !(clip > 0.0) || !(voxel_size > 0.0)) return CSN_E_ARG;               // (a NaN fails all three)
  if (n_items > 65535) return CSN_E_DIM;                                                         // one grid row per item
  if (mis8(idx) || mis8(out_offsets) || mis8(params) || mis8(bounds) || mis16(coords) || mis4(feats) || mis8(keys) ||
      (labels && (mis4(labels) || mis8(labels_out)))) return CSN_E_PTR;
  CsnPointsArgs a{};
  a.points = points; a.labels = labels; a.offsets = offsets; a.n_shapes = n_shapes; a.n_total = n_total; a.idx = idx;
  a.out_offsets = out_offsets; a.params = params; a.bounds = const_cast<double*>(bounds); a.n_items = n_items; a.max_points = max_points;
  a.sigma = sigma; a.clip = clip; a.voxel_size = voxel_size; a.coords = coords; a.feats = feats; a.labels_out = labels_out; a.keys = keys;
  a.n_out = n_out; a.status = status;
  return csn_launch_points_batch(a, (hipStream_t)stream);
}

int csn_field_index_i32(const long long* skeys, const long long* order, const long long* vid, int n_points, int n_voxels, int* home,
                        int* vox_ptr, int* vox_pts, long long* uniq_keys, int* status, void* stream) {
  if (!skeys || !order || !vid || !home || !vox_ptr || !vox_pts || !uniq_keys || !status) return CSN_E_ARG;
  if (n_points < 1 || n_voxels < 1) return CSN_E_ARG;
  if (n_voxels > n_points) return CSN_E_DIM;
  if (mis8(skeys) || mis8(order) || mis8(vid) || mis8(uniq_keys) || mis4(home) || mis4(vox_ptr) || mis4(vox_pts) || mis4(status))
    return CSN_E_PTR;
  return csn_launch_field_index(skeys, order, vid, n_points, n_voxels, home, vox_ptr, vox_pts, uniq_keys, status, (hipStream_t)stream);
}

}  // extern "C"
