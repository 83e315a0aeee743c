// Everything of the HRNet backbone that is not a convolution (MinkowskiNet/models/hrnet.py:124-131, 157-161, 308-326;
// models/modules/resnet_block.py:40-57), on point-major rows: normalise up to three maps with their BatchNorm statistics, sum
// them, add a residual, activate — forward and backward.
//
//   y = act( sum_{m < M} (gamma_m (z_m - mu_m) s_m + beta_m) + r ),  M in {1, 2, 3}, r optional, act = ReLU or identity
//
//   rows_bn_act_fwd     one pass: 64 rows per work-group, a thread owns 4 consecutive channels (16-byte accesses on every map) and
//                       keeps the terms' per-column (mu, s, gamma, beta) in registers.
//   rows_bn_act_bwd<1>  g' = dy [y > 0] (the mask is the forward's own y; identity: g' = dy), read ONCE for all M terms: writes
//                       dr = g', and per 64-row chunk the fp64 column sums of g' and of g' xhat_m.
//   rows_bn_act_sums    the chunks' sums in a fixed order (segments of the chunk list in chunk order, the segments pairwise in a
//                       fixed tree): dbeta_m = sum g' (the same for every term), dgamma_m = sum g' xhat_m, the means of the dz formula.
//   rows_bn_act_bwd<2>  dz_m = gamma_m s_m (g' - mean g' - xhat_m mean(g' xhat_m)) (training) or g' gamma_m s_m (eval).
//   bn_stats_merge      (15a) the (mean, M2) pairs that the convolution's epilogue leaves per 32-row tile, merged by Chan's formula in
//                       fp64 in a fixed order: mean, invstd, running statistics (the merge, the tile walk and the finish are
//                       rows_mma.h's, shared with rows_fc_stats; the segment count and the tree are this kernel's).
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

constexpr int MAXT = 3;

struct BnActP {
  const float* z[MAXT]; int ld_z[MAXT];
  const float* mean[MAXT]; const float* scale[MAXT]; const float* gamma[MAXT]; const float* beta[MAXT];
  float* dz[MAXT]; int ld_dz[MAXT];
  int M;
  long long n_rows; int C;
  int eval, relu; float eps;
  const float* r; int ld_r;
  float* y; int ld_y;                          // forward: written; backward: read
  const float* dy; int ld_dy;
  float* dr; int ld_dr;
  const float* coef;                           // pass 2, training: [1 + M][C] mean g', mean g' xhat_m
  double* part;                                // pass 1: [chunk][1 + M][C]
};

__device__ __forceinline__ float inv_std(const BnActP& p, int m, int c) {
  return p.eval ? 1.f / sqrtf(p.scale[m][c] + p.eps) : p.scale[m][c];
}

// Thread layout of the three row kernels: 64 rows per work-group; a thread owns 4 consecutive channels (16-byte accesses on every
// map) of every RL-th row, RL = 256 / (C / 4) row lanes (32 at C = 32, 4 at C = 256; 240 of the 256 threads work at C = 96).  A
// thread's channels never change, so the terms' per-column constants sit in registers.
struct Lane { int rl, c, RL; bool on; };
__device__ __forceinline__ Lane lane_of(int C) {
  const int c4 = C >> 2, RL = 256 / c4, rl = (int)threadIdx.x / c4;
  return Lane{rl, ((int)threadIdx.x - rl * c4) * 4, RL, rl < RL};
}

__global__ __launch_bounds__(256) void rows_bn_act_fwd_kernel(const BnActP p) {
  const Lane t = lane_of(p.C);
  if (!t.on) return;
  const long long r0 = (long long)blockIdx.x * 64;
  const int rows = (int)(p.n_rows - r0 < 64 ? p.n_rows - r0 : 64);
  float mu[MAXT][4], is[MAXT][4], ga[MAXT][4], be[MAXT][4];
#pragma unroll
  for (int m = 0; m < MAXT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = m < p.M;
      mu[m][e] = in ? p.mean[m][t.c + e] : 0.f;
      is[m][e] = in ? inv_std(p, m, t.c + e) : 0.f;
      ga[m][e] = in ? p.gamma[m][t.c + e] : 0.f;
      be[m][e] = in ? p.beta[m][t.c + e] : 0.f;
    }
#pragma unroll 2
  for (int rr = t.rl; rr < rows; rr += t.RL) {
    const long long row = r0 + rr;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (p.r) o = *reinterpret_cast<const f32x4*>(p.r + row * p.ld_r + t.c);
#pragma unroll
    for (int m = 0; m < MAXT; ++m) {
      if (m >= p.M) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.z[m] + row * p.ld_z[m] + t.c);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += fmaf(ga[m][e], (v[e] - mu[m][e]) * is[m][e], be[m][e]);
    }
    if (p.relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaxf(0.f, o[e]);
    }
    *reinterpret_cast<f32x4*>(p.y + row * p.ld_y + t.c) = o;
  }
}

// PASS 1: dr = g' and the chunk's fp64 column sums of g' and g' xhat_m: a thread adds its rows in row order, the row lanes are added
// in lane order through LDS.  PASS 2: dz_m.
template <int PASS>
__global__ __launch_bounds__(256) void rows_bn_act_bwd_kernel(const BnActP p) {
  __shared__ double sh[PASS == 1 ? (1 + MAXT) * 1024 : 1];                  // [q][row lane][C]: row lanes * C <= 1024
  const Lane t = lane_of(p.C);
  const long long r0 = (long long)blockIdx.x * 64;
  const int rows = (int)(p.n_rows - r0 < 64 ? p.n_rows - r0 : 64);
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[MAXT][4];
#pragma unroll
  for (int m = 0; m < MAXT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) s1[m][e] = 0.0;
  if (t.on) {
    float mu[MAXT][4], is[MAXT][4], gi[MAXT][4], cm[MAXT][4], c0[4];
    const bool coef = PASS == 2 && !p.eval;
#pragma unroll
    for (int e = 0; e < 4; ++e) c0[e] = coef ? p.coef[t.c + e] : 0.f;
#pragma unroll
    for (int m = 0; m < MAXT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = m < p.M;
        mu[m][e] = in ? p.mean[m][t.c + e] : 0.f;
        is[m][e] = in ? inv_std(p, m, t.c + e) : 0.f;
        gi[m][e] = in ? p.gamma[m][t.c + e] * is[m][e] : 0.f;
        cm[m][e] = (in && coef) ? p.coef[(1 + m) * p.C + t.c + e] : 0.f;
      }
#pragma unroll 2
    for (int rr = t.rl; rr < rows; rr += t.RL) {
      const long long row = r0 + rr;
      f32x4 g = *reinterpret_cast<const f32x4*>(p.dy + row * p.ld_dy + t.c);
      if (p.relu) {
        const f32x4 yv = *reinterpret_cast<const f32x4*>(p.y + row * p.ld_y + t.c);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = yv[e] > 0.f ? g[e] : 0.f;
      }
      if constexpr (PASS == 1) {
        if (p.dr) *reinterpret_cast<f32x4*>(p.dr + row * p.ld_dr + t.c) = g;
#pragma unroll
        for (int e = 0; e < 4; ++e) s0[e] += (double)g[e];
      }
#pragma unroll
      for (int m = 0; m < MAXT; ++m) {
        if (m >= p.M) continue;
        if (PASS == 2 && !p.dz[m]) continue;
        if (PASS == 2 && p.eval) {
          f32x4 d;
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = g[e] * gi[m][e];
          *reinterpret_cast<f32x4*>(p.dz[m] + row * p.ld_dz[m] + t.c) = d;
          continue;
        }
        const f32x4 zv = *reinterpret_cast<const f32x4*>(p.z[m] + row * p.ld_z[m] + t.c);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (zv[e] - mu[m][e]) * is[m][e];
          if constexpr (PASS == 1) s1[m][e] += (double)g[e] * (double)xh;
          else d[e] = gi[m][e] * (g[e] - c0[e] - xh * cm[m][e]);
        }
        if constexpr (PASS == 2) *reinterpret_cast<f32x4*>(p.dz[m] + row * p.ld_dz[m] + t.c) = d;
      }
    }
  }
  if constexpr (PASS == 1) {
    if (t.on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sh[t.rl * p.C + t.c + e] = s0[e];
#pragma unroll
        for (int m = 0; m < MAXT; ++m)
          if (m < p.M) sh[((1 + m) * t.RL + t.rl) * p.C + t.c + e] = s1[m][e];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 + p.M) * p.C; i += 256) {
      const int q = i / p.C, col = i - q * p.C;
      double s = 0.0;
      for (int k = 0; k < t.RL; ++k) s += sh[(q * t.RL + k) * p.C + col];
      p.part[((long long)blockIdx.x * (1 + p.M) + q) * p.C + col] = s;
    }
  }
}

// The tiles' (mean, M2) of a convolution's statistics epilogue -> mean, invstd, running statistics: 16 columns x 64 segments of the
// tile list per work-group; a thread merges its segment's tiles in tile order, the segments are merged pairwise in a fixed tree
// (neighbours first, the lower tiles on the left).
constexpr int SCOLS = 16, SSEG = 64;
__global__ __launch_bounds__(SCOLS * SSEG) void bn_stats_merge_kernel(const float* __restrict__ part, int n_tiles, int n_rows, int C,
                                                                       float eps, float momentum, float* __restrict__ mean,
                                                                       float* __restrict__ invstd, float* __restrict__ rmean,
                                                                       float* __restrict__ rvar) {
  __shared__ double sh[3][SSEG][SCOLS];
  const int lc = threadIdx.x % SCOLS, seg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  const int per = (n_tiles + SSEG - 1) / SSEG;
  const int t0 = seg * per, t1 = min(n_tiles, t0 + per);
  double n = 0.0, mu = 0.0, m2 = 0.0;
  chan_walk(n, mu, m2, part, t0, t1, n_rows, C, col);
  for (int stride = 1; stride < SSEG; stride <<= 1) {
    sh[0][seg][lc] = n; sh[1][seg][lc] = mu; sh[2][seg][lc] = m2;
    __syncthreads();
    if (seg % (2 * stride) == 0) chan_merge(n, mu, m2, sh[0][seg + stride][lc], sh[1][seg + stride][lc], sh[2][seg + stride][lc]);
    __syncthreads();
  }
  if (seg == 0) bn_finish(n, mu, m2, col, eps, momentum, mean, invstd, rmean, rvar);
}

struct BnSumsP {
  const double* part; int n_chunks, M, C; long long n_rows;
  float* dgamma[MAXT]; float* dbeta[MAXT];
  float* coef;                                 // [1 + M][C], may be NULL
};

// sums of the chunks' partials in a fixed order: one quantity q (blockIdx.y: 0 = sum g', 1 + m = sum g' xhat_m) of 16 columns per
// work-group; a thread adds its segment of the chunk list in chunk order, the 64 segments are added pairwise in a fixed tree
__global__ __launch_bounds__(SCOLS * SSEG) void rows_bn_act_sums_kernel(const BnSumsP p) {
  __shared__ double sh[SSEG][SCOLS];
  const int lc = threadIdx.x % SCOLS, seg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  const int q = blockIdx.y, nq = 1 + p.M;
  const int per = (p.n_chunks + SSEG - 1) / SSEG;
  const int t0 = seg * per, t1 = min(p.n_chunks, t0 + per);
  double s = 0.0;
  for (int t = t0; t < t1; ++t) s += p.part[((long long)t * nq + q) * p.C + col];
  for (int stride = 1; stride < SSEG; stride <<= 1) {
    sh[seg][lc] = s;
    __syncthreads();
    if (seg % (2 * stride) == 0) s += sh[seg + stride][lc];
    __syncthreads();
  }
  if (seg != 0) return;
  if (p.coef) p.coef[q * p.C + col] = (float)(s / (double)p.n_rows);
#pragma unroll
  for (int m = 0; m < MAXT; ++m) {
    if (m >= p.M) continue;
    if (q == 0 && p.dbeta[m]) p.dbeta[m][col] = (float)s;
    if (q == 1 + m && p.dgamma[m]) p.dgamma[m][col] = (float)s;
  }
}

struct WsLayout { long long part, coef, total; };
WsLayout ws_layout(long long n_rows, int C, int M) {
  WsLayout L{};
  long long o = 0;
  L.part = o; o += up256(((n_rows + 63) / 64) * (1 + M) * C * (long long)sizeof(double));
  L.coef = o; o += up256((long long)(1 + M) * C * (long long)sizeof(float));
  L.total = o;
  return L;
}

BnActP make_p(const CsnRowsBnActArgs& a) {
  BnActP p{};
  for (int m = 0; m < a.n_terms; ++m) {
    p.z[m] = a.z[m]; p.ld_z[m] = a.ld_z[m]; p.mean[m] = a.mean[m]; p.scale[m] = a.scale[m]; p.gamma[m] = a.gamma[m];
    p.beta[m] = a.beta[m]; p.dz[m] = a.dz[m]; p.ld_dz[m] = a.ld_dz[m];
  }
  p.M = a.n_terms; p.n_rows = a.n_rows; p.C = a.C; p.eval = !a.training; p.relu = a.relu; p.eps = a.eps;
  p.r = a.r; p.ld_r = a.ld_r; p.y = a.y; p.ld_y = a.ld_y; p.dy = a.dy; p.ld_dy = a.ld_dy; p.dr = a.dr; p.ld_dr = a.ld_dr;
  return p;
}

}  // namespace

long long csn_rows_bn_act_ws_bytes(long long n_rows, int C, int n_terms) { return ws_layout(n_rows, C, n_terms).total; }

int csn_launch_bn_stats_merge(const float* part, int n_tiles, int n_rows, int C, float eps, float momentum, float* mean, float* invstd,
                              float* running_mean, float* running_var, hipStream_t st) {
  hipLaunchKernelGGL(bn_stats_merge_kernel, dim3(C / SCOLS), dim3(SCOLS * SSEG), 0, st, part, n_tiles, n_rows, C, eps, momentum, mean,
                     invstd, running_mean, running_var);
  return (int)hipGetLastError();
}

int csn_launch_rows_bn_act_fwd(const CsnRowsBnActArgs& a, hipStream_t st) {
  const BnActP p = make_p(a);
  const unsigned n_chunks = (unsigned)(((long long)a.n_rows + 63) / 64);
  hipLaunchKernelGGL(rows_bn_act_fwd_kernel, dim3(n_chunks), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

int csn_launch_rows_bn_act_bwd(const CsnRowsBnActArgs& a, hipStream_t st) {
  const WsLayout L = ws_layout(a.n_rows, a.C, a.n_terms);
  char* ws = static_cast<char*>(a.ws);
  BnActP p = make_p(a);
  p.part = reinterpret_cast<double*>(ws + L.part);
  float* coef = reinterpret_cast<float*>(ws + L.coef);
  p.coef = coef;
  const int n_chunks = (int)(((long long)a.n_rows + 63) / 64);
  bool any_dz = false, any_sum = false;
  for (int m = 0; m < a.n_terms; ++m) {
    any_dz |= a.dz[m] != nullptr;
    any_sum |= a.dgamma[m] != nullptr || a.dbeta[m] != nullptr;
  }
  const bool need_coef = any_dz && a.training;
  if (a.dr || any_sum || need_coef) {
    hipLaunchKernelGGL(rows_bn_act_bwd_kernel<1>, dim3(n_chunks), dim3(256), 0, st, p);
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (any_sum || need_coef) {
    BnSumsP s{};
    s.part = p.part; s.n_chunks = n_chunks; s.M = a.n_terms; s.C = a.C; s.n_rows = a.n_rows; s.coef = need_coef ? coef : nullptr;
    for (int m = 0; m < a.n_terms; ++m) { s.dgamma[m] = a.dgamma[m]; s.dbeta[m] = a.dbeta[m]; }
    hipLaunchKernelGGL(rows_bn_act_sums_kernel, dim3(a.C / SCOLS, 1 + a.n_terms), dim3(SCOLS * SSEG), 0, st, s);
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (any_dz) {
    hipLaunchKernelGGL(rows_bn_act_bwd_kernel<2>, dim3(n_chunks), dim3(256), 0, st, p);
    if (const int e = (int)hipGetLastError()) return e;
  }
  return 0;
}
