// fc_layer of the MinkowskiNet CSN head on point-major rows (MinkowskiNet/models/hrnet.py:332-339, applied at :439 and :451):
// a kernel-size-1 convolution with bias, BatchNorm over the rows of the call, ReLU — forward (training / eval) and backward.
//
//   rows_gemm          C[M][J] = A[M][K] * B, A rows from global memory straight into the matrix-core operand (a lane owns one
//                      row and 4 / 8 consecutive k), B (the weight, [J][K] or [K][J]) staged through LDS once per work-group.
//                      A wave owns 32 rows x NB * 32 columns, so a column's 32 values sit in one lane pair and the BatchNorm
//                      partials (mean, M2 of the wave's rows) fall out of the accumulators.  Epilogues: z = acc + bias (with or
//                      without the partials), or the folded eval form max(0, acc * s + t).  The same kernel forms dx = dz * w.
//                      The B staging, the contraction step and the bias / store / partials epilogue are rows_mma.h's.
//   rows_fc_stats      merges the per-tile (count, mean, M2) triples by Chan's formula in fp64 in a fixed order: mean, invstd,
//                      running statistics.
//   rows_fc_apply      y = max(0, gamma * (z - mean) * invstd + beta).
//   rows_fc_bwd<PASS>  pass 1: per-chunk fp64 sums of g' and g' * xhat; pass 2: dz (written) and its per-chunk column sums.
//   rows_fc_bwd_sums   the chunks' sums in a fixed order: dgamma, dbeta, the two means of the dz formula.
//   rows_colsum / rows_colsum_merge   fp64 column sums of 64-row chunks and their sum in chunk order: dbias here (the chunks
//                      are pass 2's) and of the sparse convolution (csn_launch_rows_colsum*).
//   rows_fc_wgrad      dw = dz^T * x: both operands are k-major (the contraction runs over the rows), so a lane reads its 8
//                      contraction steps as 8 rows of one column — 32 lanes of a half wave read one contiguous 128-byte run per
//                      row — and splits them in registers: no LDS image, no transpose.  Rows past the end read as zero through the
//                      buffer range check (never a lane mask).  The four waves of a work-group contract a quarter of its row
//                      chunk each and are added through LDS in wave order; chunks are split-K slabs added by csn_launch_slab_reduce.
//                      The 16-row step and the reduction are rows_mma.h's; the kernel keeps its addressing.
//   rows_gemm16 / rows_fc_wgrad16   the same bodies with ONE 16-bit product per operand pair (math modes 2 bf16 / 3 fp16 behind
//                      csn_set_thread_rows16; fp16: the forward products alone): operands rounded once, the weight converted when it
//                      is stored to LDS.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

struct RowsGemmP {
  const float* a; int lda;            // A[M][K]
  const float* b; int ldb;            // B_KN ? B[K][J] : B[J][K]
  float* c; int ldc;                  // C[M][J]
  int M, K, J;
  int epi;                            // 0: acc (+ bias); 1: acc + bias and the tiles' (mean, M2); 2: max(0, acc * s + t) (eval)
  const float* bias;
  float* part;                        // epi 1: [tile][2][J], tile = 32 rows
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps;
};

// the body of rows_gemm_kernel (MODE 0 / 1) and rows_gemm16_kernel (MODE 2 bf16 / 3 fp16: one product, the tile holds shorts)
template <int NB, int MODE, bool B_KN>
__device__ __forceinline__ void rows_gemm_body(const RowsGemmP p) {
  __shared__ __attribute__((aligned(16))) bs_t<MODE> Bs[NB * 32 * bs_pitch<MODE>];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  const long long row_g = (long long)rg * 128;                        // first row of the work-group
  const long long rows_left = p.M - row_g;                            // >= 1
  const csn_rsrc_t ar = csn_make_rsrc(p.a + row_g * p.lda, ((rows_left - 1) * p.lda + p.K) * 4LL);
  const unsigned a_off = (unsigned)(((wave * 32 + li) * p.lda + (MODE == 0 ? 4 : 8) * h) * 4);

  f32x16 acc[NB] = {};
  f32x4 an[4], bn[NB];
  auto load_a = [&](int k0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, a_off + (unsigned)((k0 + a_kofs<MODE>(g)) * 4));
  };

  load_a(0);
  load_b<NB, B_KN>(bn, p.b, p.ldb, 0, j0, p.J, tid);
  for (int k0 = 0; k0 < p.K; k0 += 32) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, B_KN, MODE>(Bs, bn, tid);
    f32x4 af[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = an[g];
    __syncthreads();
    if (k0 + 32 < p.K) { load_a(k0 + 32); load_b<NB, B_KN>(bn, p.b, p.ldb, k0 + 32, j0, p.J, tid); }
    mma_step<NB, MODE>(acc, af, Bs, li, h);
  }

  const long long row_w = row_g + wave * 32;                          // first row of the wave's tile
  const int cnt = (int)(p.M - row_w < 32 ? (p.M - row_w < 0 ? 0 : p.M - row_w) : 32);
  const long long tile = (long long)rg * 4 + wave;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = j0 + nb * 32 + li;
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    if (p.epi == 2) {
      const float s = p.gamma[col] / sqrtf(p.rvar[col] + p.eps);
      const float t = p.beta[col] + ((p.bias ? p.bias[col] : 0.f) - p.rmean[col]) * s;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = csn_acc_row(r, h);                             // = csn_acc_row(r, 0) + 4 h: store_tile's address form below
        if (rr < cnt) (p.c + (row_w + csn_acc_row(r, 0)) * p.ldc)[4 * h * p.ldc + col] = fmaxf(0.f, fmaf(acc[nb][r], s, t));
      }
      continue;
    }
    store_tile(acc[nb], p.bias ? p.bias[col] : 0.f, p.c, p.ldc, row_w, cnt, col, h, p.epi == 1, p.part, tile, p.J);
  }
}

template <int NB, int MODE, bool B_KN>
__global__ __launch_bounds__(256) void rows_gemm_kernel(const RowsGemmP p) { rows_gemm_body<NB, MODE, B_KN>(p); }

// the single-product instances: H16 = fp16 operands (forward only), else bf16
template <int NB, bool H16, bool B_KN>
__global__ __launch_bounds__(256) void rows_gemm16_kernel(const RowsGemmP p) { rows_gemm_body<NB, H16 ? 3 : 2, B_KN>(p); }

// one thread per (column, segment of the tiles): 32 columns x NSEG segments per work-group, segments merged in order by segment 0
constexpr int NSEG = 32;
__global__ __launch_bounds__(32 * NSEG) void rows_fc_stats_kernel(const float* __restrict__ part, int n_tiles, int n_rows, int C, float eps,
                                                            float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                            float* __restrict__ rmean, float* __restrict__ rvar) {
  __shared__ double sh[3][NSEG][32];
  const int lc = threadIdx.x & 31, seg = threadIdx.x >> 5, col = blockIdx.x * 32 + lc;
  const int per = (n_tiles + NSEG - 1) / NSEG;
  const int t0 = seg * per, t1 = min(n_tiles, t0 + per);
  double n = 0.0, mu = 0.0, m2 = 0.0;
  chan_walk(n, mu, m2, part, t0, t1, n_rows, C, col);
  sh[0][seg][lc] = n; sh[1][seg][lc] = mu; sh[2][seg][lc] = m2;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < NSEG; ++s) chan_merge(n, mu, m2, sh[0][s][lc], sh[1][s][lc], sh[2][s][lc]);
  bn_finish(n, mu, m2, col, eps, momentum, mean, invstd, rmean, rvar);
}

__global__ __launch_bounds__(256) void rows_fc_apply_kernel(const float* __restrict__ z, int ldz, float* __restrict__ y, int ldy,
                                                            long long n_rows, int C, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta) {
  const int c4 = C >> 2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_rows * c4) return;
  const long long row = idx / c4;
  const int c = (int)(idx - row * c4) * 4;
  const f32x4 v = *reinterpret_cast<const f32x4*>(z + row * ldz + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaxf(0.f, fmaf(gamma[c + e], (v[e] - mean[c + e]) * invstd[c + e], beta[c + e]));
  *reinterpret_cast<f32x4*>(y + row * ldy + c) = o;
}

struct RowsBwdP {
  const float* dy; int ld_dy;
  const float* y; int ld_y;
  const float* z; int ld_z;
  long long n_rows; int C;
  const float* mean; const float* scale;     // training: invstd; eval: the running variance (invstd = 1 / sqrt(var + eps))
  int eval; float eps;
  const float* gamma;
  const float* coef;                         // pass 2, training: [2][C] mean_n g', mean_n g' xhat
  float* dz;                                 // pass 2: [n_rows][C]
  double* part;                              // [chunk][NQ][C]
};

// 64 rows per work-group; a lane owns a column (256-byte row segments per wave), the four waves take every fourth row and are
// added in wave order
template <int PASS>
__global__ __launch_bounds__(256) void rows_fc_bwd_kernel(const RowsBwdP p) {
  constexpr int NQ = PASS == 1 ? 2 : 1;
  __shared__ double sh[NQ][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * 64;
  const long long r1 = r0 + 64 < p.n_rows ? r0 + 64 : p.n_rows;
  for (int cb = 0; cb * 64 < p.C; ++cb) {
    const int c = cb * 64 + lane;
    const bool ok = c < p.C;
    double s0 = 0.0, s1 = 0.0;
    if (ok) {
      const float mu = p.mean[c];
      const float is = p.eval ? 1.f / sqrtf(p.scale[c] + p.eps) : p.scale[c];
      const float gi = p.gamma[c] * is;
      float c1 = 0.f, c2 = 0.f;
      if (PASS == 2 && !p.eval) { c1 = p.coef[c]; c2 = p.coef[p.C + c]; }
      for (long long r = r0 + w; r < r1; r += 4) {
        const float g = p.y[r * p.ld_y + c] > 0.f ? p.dy[r * p.ld_dy + c] : 0.f;
        const float xh = (p.z[r * p.ld_z + c] - mu) * is;
        if constexpr (PASS == 1) {
          s0 += (double)g;
          s1 += (double)g * (double)xh;
        } else {
          const float d = p.eval ? g * gi : gi * (g - c1 - xh * c2);
          p.dz[r * p.C + c] = d;
          s0 += (double)d;
        }
      }
    }
    sh[0][w][lane] = s0;
    if constexpr (NQ == 2) sh[1][w][lane] = s1;
    __syncthreads();
    if (w == 0 && ok && p.part) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        p.part[((long long)blockIdx.x * NQ + q) * p.C + c] = ((sh[q][0][lane] + sh[q][1][lane]) + sh[q][2][lane]) + sh[q][3][lane];
    }
    __syncthreads();
  }
}

// sums of the chunks' partials in a fixed order (32 columns x NSEG segments, as rows_fc_stats_kernel):
// q0 = sum g' -> dbeta, coef[0]; q1 = sum g' xhat -> dgamma, coef[1]
__global__ __launch_bounds__(32 * NSEG) void rows_fc_bwd_sums_kernel(const double* __restrict__ part, int n_chunks, int C, long long n_rows,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ coef) {
  __shared__ double sh[2][NSEG][32];
  const int lc = threadIdx.x & 31, seg = threadIdx.x >> 5, col = blockIdx.x * 32 + lc;
  const int per = (n_chunks + NSEG - 1) / NSEG;
  const int t0 = seg * per, t1 = min(n_chunks, t0 + per);
  double s[2] = {0.0, 0.0};
  for (int t = t0; t < t1; ++t)
    for (int q = 0; q < 2; ++q) s[q] += part[((long long)t * 2 + q) * C + col];
  sh[0][seg][lc] = s[0]; sh[1][seg][lc] = s[1];
  __syncthreads();
  if (seg != 0) return;
  for (int k = 1; k < NSEG; ++k) { s[0] += sh[0][k][lc]; s[1] += sh[1][k][lc]; }
  if (dgamma) dgamma[col] = (float)s[1];
  if (dbeta) dbeta[col] = (float)s[0];
  if (coef) { coef[col] = (float)(s[0] / (double)n_rows); coef[C + col] = (float)(s[1] / (double)n_rows); }
}

// fp64 column sums of 64-row chunks of x: a lane owns a column, the four waves take every fourth row and are added in wave order
__global__ __launch_bounds__(256) void rows_colsum_kernel(const float* __restrict__ x, int ldx, long long n_rows, int C,
                                                          double* __restrict__ part) {
  __shared__ double sh[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * 64;
  const long long r1 = r0 + 64 < n_rows ? r0 + 64 : n_rows;
  for (int cb = 0; cb * 64 < C; ++cb) {
    const int c = cb * 64 + lane;
    const bool ok = c < C;
    double s = 0.0;
    if (ok)
      for (long long r = r0 + w; r < r1; r += 4) s += (double)x[r * ldx + c];
    sh[w][lane] = s;
    __syncthreads();
    if (w == 0 && ok) part[(long long)blockIdx.x * C + c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    __syncthreads();
  }
}

// the chunks' [chunk][C] sums in chunk order: 32 columns x NSEG segments of the chunk list per work-group, segments added in order
__global__ __launch_bounds__(32 * NSEG) void rows_colsum_merge_kernel(const double* __restrict__ part, int n_chunks, int C,
                                                                float* __restrict__ out) {
  __shared__ double sh[NSEG][32];
  const int lc = threadIdx.x & 31, seg = threadIdx.x >> 5, col = blockIdx.x * 32 + lc;
  const int per = (n_chunks + NSEG - 1) / NSEG;
  const int t0 = seg * per, t1 = min(n_chunks, t0 + per);
  double s = 0.0;
  for (int t = t0; t < t1; ++t) s += part[(long long)t * C + col];
  sh[seg][lc] = s;
  __syncthreads();
  if (seg != 0) return;
  for (int k = 1; k < NSEG; ++k) s += sh[k][lc];
  out[col] = (float)s;
}

// dw[co][ci] = sum_n dz[n][co] x[n][ci] over the rows of one split-K chunk; see the file header
// the body of rows_fc_wgrad_kernel (MODE 0 / 1) and rows_fc_wgrad16_kernel (MODE 2: one bf16 product)
template <int TA, int MODE>
__device__ __forceinline__ void rows_fc_wgrad_body(const float* __restrict__ dz, int ldz, const float* __restrict__ x, int ldx,
                                                   float* __restrict__ out, long long n_rows, int c_out, int c_in, int chunk) {
  __shared__ float red[TA * WG_TB * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 32 * TA;
  const int nbv = (c_in - ci0) >= 64 ? 2 : 1;                         // column blocks of x inside c_in (c_in % 32 == 0)
  const int quarter = chunk >> 2;                                     // chunk % 64 == 0
  const long long rb = (long long)blockIdx.z * chunk + (long long)wave * quarter;
  const long long left = n_rows - rb;
  const csn_rsrc_t zr = csn_make_rsrc(dz + rb * ldz, left > 0 ? ((left - 1) * ldz + c_out) * 4LL : 0LL);
  const csn_rsrc_t xr = csn_make_rsrc(x + rb * ldx, left > 0 ? ((left - 1) * ldx + c_in) * 4LL : 0LL);

  f32x16 acc[TA][WG_TB] = {};
  float an[TA][8], bn[WG_TB][8];
  auto load = [&](int rr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + wgrad_row<MODE>(h, e);
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) an[ta][e] = csn_bload(zr, (unsigned)((row * ldz + co0 + ta * 32 + li) * 4));
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bn[tb][e] = tb < nbv ? csn_bload(xr, (unsigned)((row * ldx + ci0 + tb * 32 + li) * 4)) : 0.f;
    }
  };
  const int n_steps = wgrad_steps(left, quarter);
  if (n_steps > 0) load(0);
  for (int st = 0; st < n_steps; ++st) {
    float af[TA][8], bf[WG_TB][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) af[ta][e] = an[ta][e];
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bf[tb][e] = bn[tb][e];
    }
    if (st + 1 < n_steps) load((st + 1) * 16);
    wgrad_step<TA, MODE, false>(acc, af, bf, nbv);
  }
  wgrad_reduce_store<TA>(acc, red, out + (long long)blockIdx.z * c_out * c_in, c_in, co0, ci0, nbv, wave, l);
}

template <int TA, int MODE>
__global__ __launch_bounds__(256) void rows_fc_wgrad_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ x, int ldx,
                                                            float* __restrict__ out, long long n_rows, int c_out, int c_in, int chunk) {
  rows_fc_wgrad_body<TA, MODE>(dz, ldz, x, ldx, out, n_rows, c_out, c_in, chunk);
}

template <int TA>
__global__ __launch_bounds__(256) void rows_fc_wgrad16_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ x, int ldx,
                                                              float* __restrict__ out, long long n_rows, int c_out, int c_in, int chunk) {
  rows_fc_wgrad_body<TA, 2>(dz, ldz, x, ldx, out, n_rows, c_out, c_in, chunk);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline int wgrad_ta(int c_out) { return c_out == 96 ? 3 : (c_out >= 128 ? 4 : c_out / 32); }

// split-K of the weight gradient: about one work-group per CU, chunks of a multiple of 64 rows and at most 65536 (a wave's
// quarter stays far below the 2 GiB buffer window)
void wgrad_split(long long n_rows, int c_in, int c_out, int& splits, int& chunk) {
  const long long tiles = (long long)((c_in + 63) / 64) * (c_out / (32 * wgrad_ta(c_out)));
  long long want = (256 + tiles - 1) / tiles;
  long long ch = ((n_rows + want - 1) / want + 63) / 64 * 64;
  if (ch > 65536) ch = 65536;
  chunk = (int)ch;
  splits = (int)((n_rows + ch - 1) / ch);
}

struct WsLayout { long long part, dz, ztmp, coef, slabs, total; };

WsLayout ws_layout(long long n_rows, int c_in, int c_out, int training, int backward) {
  WsLayout L{};
  long long o = 0;
  if (!backward) {
    L.part = o;
    if (training) o += up256(((n_rows + 127) / 128) * 4 * 2 * c_out * (long long)sizeof(float));
    L.total = o;
    return L;
  }
  L.part = o;  o += up256(((n_rows + 63) / 64) * 2 * c_out * (long long)sizeof(double));
  L.dz = o;    o += up256(n_rows * c_out * (long long)sizeof(float));
  L.ztmp = o;  if (!training) o += up256(n_rows * c_out * (long long)sizeof(float));
  L.coef = o;  o += up256(2LL * c_out * (long long)sizeof(float));
  int splits, chunk;
  wgrad_split(n_rows, c_in, c_out, splits, chunk);
  L.slabs = o; if (splits > 1) o += up256((long long)splits * c_out * c_in * (long long)sizeof(float));
  L.total = o;
  return L;
}

template <int NB, bool B_KN>
int launch_gemm_nb(const RowsGemmP& p, int mode, hipStream_t st) {
  // the fp16 product exists for the forward ([J][K] weights) alone
  void (*const k[4])(RowsGemmP) = {rows_gemm_kernel<NB, 0, B_KN>, rows_gemm_kernel<NB, 1, B_KN>, rows_gemm16_kernel<NB, false, B_KN>,
                                   B_KN ? nullptr : rows_gemm16_kernel<NB, true, false>};
  return launch_row_product(k, p, NB, mode, st);
}

// forward products: the wave owns every column up to 128, two column groups at 256
int launch_fwd_gemm(const RowsGemmP& p, int mode, hipStream_t st) {
  return dispatch4(p.J / 32, [&](auto nb) { return launch_gemm_nb<nb(), false>(p, mode, st); });
}

template <int TA>
int launch_wgrad_ta(const float* dz, const float* x, int ldx, float* out, long long n_rows, int c_in, int c_out, int splits, int chunk,
                    int mode, hipStream_t st) {
  const dim3 grid((unsigned)((c_in + 63) / 64), (unsigned)(c_out / (32 * TA)), (unsigned)splits), block(256);
  auto* const k = mode == 0 ? rows_fc_wgrad_kernel<TA, 0> : (mode == 1 ? rows_fc_wgrad_kernel<TA, 1> : rows_fc_wgrad16_kernel<TA>);
  hipLaunchKernelGGL(k, grid, block, 0, st, dz, c_out, x, ldx, out, n_rows, c_out, c_in, chunk);
  return (int)hipGetLastError();
}

}  // namespace

long long csn_rows_fc_ws_bytes(long long n_rows, int c_in, int c_out, int training, int backward) {
  return ws_layout(n_rows, c_in, c_out, training, backward).total;
}

int csn_launch_rows_colsum(const float* x, int ldx, long long n_rows, int C, double* part, hipStream_t st) {
  hipLaunchKernelGGL(rows_colsum_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(256), 0, st, x, ldx, n_rows, C, part);
  return (int)hipGetLastError();
}

int csn_launch_rows_colsum_merge(const double* part, int n_chunks, int C, float* out, hipStream_t st) {
  hipLaunchKernelGGL(rows_colsum_merge_kernel, dim3(C / 32), dim3(32 * NSEG), 0, st, part, n_chunks, C, out);
  return (int)hipGetLastError();
}

// mode: 0 fp32, 1 bf16x3, 2 bf16 / 3 fp16 single product (csn_capi.hip resolves the thread's math mode and rows16 flag)
int csn_launch_rows_fc_fwd(const CsnRowsFcArgs& a, int mode, hipStream_t st) {
  const WsLayout L = ws_layout(a.n_rows, a.c_in, a.c_out, a.training, 0);
  RowsGemmP p{};
  p.a = a.x; p.lda = a.ld_x; p.b = a.w; p.ldb = a.c_in; p.M = a.n_rows; p.K = a.c_in; p.J = a.c_out;
  p.bias = a.bias; p.gamma = a.gamma; p.beta = a.beta; p.rmean = a.running_mean; p.rvar = a.running_var; p.eps = a.eps;
  if (!a.training) {
    p.c = a.y; p.ldc = a.ld_y; p.epi = 2;
    return launch_fwd_gemm(p, mode, st);
  }
  p.c = a.z; p.ldc = a.ld_z; p.epi = 1;
  p.part = reinterpret_cast<float*>(static_cast<char*>(a.ws) + L.part);
  if (const int e = launch_fwd_gemm(p, mode, st)) return e;
  const int n_tiles = (int)(((long long)a.n_rows + 127) / 128) * 4;
  hipLaunchKernelGGL(rows_fc_stats_kernel, dim3(a.c_out / 32), dim3(32 * NSEG), 0, st, p.part, n_tiles, a.n_rows, a.c_out, a.eps, a.momentum,
                     a.mean, a.invstd, a.running_mean, a.running_var);
  if (const int e = (int)hipGetLastError()) return e;
  const long long quads = (long long)a.n_rows * (a.c_out / 4);
  hipLaunchKernelGGL(rows_fc_apply_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, a.z, a.ld_z, a.y, a.ld_y,
                     (long long)a.n_rows, a.c_out, a.mean, a.invstd, a.gamma, a.beta);
  return (int)hipGetLastError();
}

int csn_launch_rows_fc_bwd(const CsnRowsFcArgs& a, int mode, hipStream_t st) {
  if (mode == 3) return -1;                                           // fp16 is forward only
  const WsLayout L = ws_layout(a.n_rows, a.c_in, a.c_out, a.training, 1);
  char* ws = static_cast<char*>(a.ws);
  double* part = reinterpret_cast<double*>(ws + L.part);
  float* dz = reinterpret_cast<float*>(ws + L.dz);
  float* coef = reinterpret_cast<float*>(ws + L.coef);
  const float* z = a.z;
  int ld_z = a.ld_z;
  if (!a.training) {
    // eval kept no z: the product again, z = x w^T + bias
    RowsGemmP g{};
    g.a = a.x; g.lda = a.ld_x; g.b = a.w; g.ldb = a.c_in; g.M = a.n_rows; g.K = a.c_in; g.J = a.c_out;
    g.c = reinterpret_cast<float*>(ws + L.ztmp); g.ldc = a.c_out; g.epi = 0; g.bias = a.bias;
    if (const int e = launch_fwd_gemm(g, mode, st)) return e;
    z = g.c; ld_z = a.c_out;
  }
  const int n_chunks = (int)(((long long)a.n_rows + 63) / 64);
  RowsBwdP b{};
  b.dy = a.dy; b.ld_dy = a.ld_dy; b.y = a.y; b.ld_y = a.ld_y; b.z = z; b.ld_z = ld_z; b.n_rows = a.n_rows; b.C = a.c_out;
  b.mean = a.mean; b.scale = a.invstd; b.eval = !a.training; b.eps = a.eps; b.gamma = a.gamma; b.coef = coef; b.dz = dz; b.part = part;
  hipLaunchKernelGGL(rows_fc_bwd_kernel<1>, dim3(n_chunks), dim3(256), 0, st, b);
  if (const int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(rows_fc_bwd_sums_kernel, dim3(a.c_out / 32), dim3(32 * NSEG), 0, st, part, n_chunks, a.c_out, (long long)a.n_rows, a.dgamma,
                     a.dbeta, coef);
  if (const int e = (int)hipGetLastError()) return e;
  if (!a.dx && !a.dw && !a.dbias) return 0;
  if (!a.dbias) b.part = nullptr;
  hipLaunchKernelGGL(rows_fc_bwd_kernel<2>, dim3(n_chunks), dim3(256), 0, st, b);
  if (const int e = (int)hipGetLastError()) return e;
  if (a.dbias)
    if (const int e = csn_launch_rows_colsum_merge(part, n_chunks, a.c_out, a.dbias, st)) return e;
  if (a.dx) {
    RowsGemmP g{};
    g.a = dz; g.lda = a.c_out; g.b = a.w; g.ldb = a.c_in; g.M = a.n_rows; g.K = a.c_out; g.J = a.c_in;
    g.c = a.dx; g.ldc = a.ld_dx; g.epi = 0;
    if (const int e = launch_gemm_nb<4, true>(g, mode, st)) return e;
  }
  if (a.dw) {
    int splits, chunk;
    wgrad_split(a.n_rows, a.c_in, a.c_out, splits, chunk);
    float* out = splits > 1 ? reinterpret_cast<float*>(ws + L.slabs) : a.dw;
    const int e = dispatch4(wgrad_ta(a.c_out), [&](auto ta) {
      return launch_wgrad_ta<ta()>(dz, a.x, a.ld_x, out, a.n_rows, a.c_in, a.c_out, splits, chunk, mode, st);
    });
    if (e) return e;
    if (splits > 1) return csn_launch_slab_reduce(out, a.dw, splits, (long long)a.c_out * a.c_in, 1.f, 0, st);
  }
  return 0;
}
