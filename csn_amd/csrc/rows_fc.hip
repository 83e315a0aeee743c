// fc_layer of the MinkowskiNet CSN head on point-major rows (MinkowskiNet/models/hrnet.py:332-339, applied at :439 and :451):
// a kernel-size-1 convolution with bias, BatchNorm over the rows of the call, ReLU — forward (training / eval) and backward.
//
//   rows_gemm          C[M][J] = A[M][K] * B, A rows from global memory straight into the matrix-core operand (a lane owns one
//                      row and 4 / 8 consecutive k), B (the weight, [J][K] or [K][J]) staged through LDS once per work-group.
//                      A wave owns 32 rows x NB * 32 columns, so a column's 32 values sit in one lane pair and the BatchNorm
//                      partials (mean, M2 of the wave's rows) fall out of the accumulators.  Epilogues: z = acc + bias (with or
//                      without the partials), or the folded eval form max(0, acc * s + t).  The same kernel forms dx = dz * w.
//   rows_fc_stats      merges the per-tile (count, mean, M2) triples by Chan's formula in fp64 in a fixed order: mean, invstd,
//                      running statistics.
//   rows_fc_apply      y = max(0, gamma * (z - mean) * invstd + beta).
//   rows_fc_bwd<PASS>  pass 1: per-chunk fp64 sums of g' and g' * xhat; pass 2: dz (written) and its per-chunk column sums.
//   rows_fc_bwd_sums   the chunks' sums in a fixed order: dgamma, dbeta, the two means of the dz formula; dbias.
//   rows_fc_wgrad      dw = dz^T * x: both operands are k-major (the contraction runs over the rows), so a lane reads its 8
//                      contraction steps as 8 rows of one column — 32 lanes of a half wave read one contiguous 128-byte run per
//                      row — and splits them in registers: no LDS image, no transpose.  Rows past the end read as zero through the
//                      buffer range check (never a lane mask).  The four waves of a work-group contract a quarter of its row
//                      chunk each and are added through LDS in wave order; chunks are split-K slabs added by csn_launch_slab_reduce.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "csn_kernels.h"

namespace {
using namespace csn_mode;

constexpr int BS_PITCH = 36;          // floats per LDS row of the B tile: 32 k + 4 (16-byte reads of 16 lanes hit 16 x 4 distinct banks)

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

template <int NB, int MODE, bool B_KN>
__global__ __launch_bounds__(256) void rows_gemm_kernel(const RowsGemmP p) {
  __shared__ __attribute__((aligned(16))) float Bs[NB * 32 * BS_PITCH];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  const long long row_g = (long long)rg * 128;                        // first row of the work-group
  const long long rows_left = p.M - row_g;                            // >= 1
  const csn_rsrc_t ar = csn_make_rsrc(p.a + row_g * p.lda, ((rows_left - 1) * p.lda + p.K) * 4LL);
  const unsigned a_off = (unsigned)(((wave * 32 + li) * p.lda + (MODE == 0 ? 4 : 8) * h) * 4);

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

  f32x4 an[4], bn[NB];
  auto load_a = [&](int k0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // mode 0: k = k0 + 8 g + 4 h + t; 16-bit: k = k0 + 16 (g / 2) + 8 h + 4 (g % 2) + t
      const int kofs = MODE == 0 ? 8 * g : 16 * (g >> 1) + 4 * (g & 1);
      an[g] = csn_bload4(ar, a_off + (unsigned)((k0 + kofs) * 4));
    }
  };
  auto load_b = [&](int k0) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = tid + 256 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if constexpr (!B_KN) {
        const int j = idx >> 3, kq = idx & 7;
        if (j0 + j < p.J) v = *reinterpret_cast<const f32x4*>(p.b + (long long)(j0 + j) * p.ldb + k0 + 4 * kq);
      } else {
        const int k = idx / (NB * 8), jq = idx % (NB * 8);
        if (j0 + 4 * jq < p.J) v = *reinterpret_cast<const f32x4*>(p.b + (long long)(k0 + k) * p.ldb + j0 + 4 * jq);
      }
      bn[u] = v;
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = tid + 256 * u;
      if constexpr (!B_KN) {
        const int j = idx >> 3, kq = idx & 7;
        *reinterpret_cast<f32x4*>(&Bs[j * BS_PITCH + 4 * kq]) = bn[u];
      } else {
        const int k = idx / (NB * 8), jq = idx % (NB * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(4 * jq + e) * BS_PITCH + k] = bn[u][e];
      }
    }
  };

  load_a(0);
  load_b(0);
  for (int k0 = 0; k0 < p.K; k0 += 32) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b();
    f32x4 af[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = an[g];
    __syncthreads();
    if (k0 + 32 < p.K) { load_a(k0 + 32); load_b(k0 + 32); }
    if constexpr (MODE == 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const f32x4 bq = *reinterpret_cast<const f32x4*>(&Bs[(nb * 32 + li) * BS_PITCH + 8 * g + 4 * h]);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[nb] = csn_mfma(af[g][t], bq[t], acc[nb]);
        }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        s16x4 h0, l0, h1, l1;
        split4<Bf16x3>(af[2 * s2], h0, l0);
        split4<Bf16x3>(af[2 * s2 + 1], h1, l1);
        const s16x8 ahi = join8(h0, h1), alo = join8(l0, l1);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const float* bp = &Bs[(nb * 32 + li) * BS_PITCH + 16 * s2 + 8 * h];
          split4<Bf16x3>(*reinterpret_cast<const f32x4*>(bp), h0, l0);
          split4<Bf16x3>(*reinterpret_cast<const f32x4*>(bp + 4), h1, l1);
          const s16x8 bhi = join8(h0, h1), blo = join8(l0, l1);
          acc[nb] = mfma32<false>(alo, bhi, acc[nb]);
          acc[nb] = mfma32<false>(ahi, blo, acc[nb]);
          acc[nb] = mfma32<false>(ahi, bhi, acc[nb]);
        }
      }
    }
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
        const int rr = csn_acc_row(r, h);
        if (rr < cnt) p.c[(row_w + rr) * p.ldc + col] = fmaxf(0.f, fmaf(acc[nb][r], s, t));
      }
      continue;
    }
    const float bv = p.bias ? p.bias[col] : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = csn_acc_row(r, h);
      const float v = acc[nb][r] + bv;
      acc[nb][r] = v;
      if (rr < cnt) { p.c[(row_w + rr) * p.ldc + col] = v; sum += v; }
    }
    if (p.epi == 1) {
      // (mean, M2) of the wave's cnt rows, two passes over the registers: no cancellation
      sum += csn_xhalf(sum);
      const float mu = cnt > 0 ? sum / (float)cnt : 0.f;
      float m2 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = acc[nb][r] - mu;
        if (csn_acc_row(r, h) < cnt) m2 = fmaf(d, d, m2);
      }
      m2 += csn_xhalf(m2);
      if (h == 0) {
        p.part[(tile * 2) * p.J + col] = mu;
        p.part[(tile * 2 + 1) * p.J + col] = m2;
      }
    }
  }
}

// Chan's merge of (n, mean, M2) pairs
__device__ __forceinline__ void chan_merge(double& n, double& mu, double& m2, double nb, double mb, double qb) {
  if (nb <= 0.0) return;
  const double nn = n + nb, d = mb - mu;
  mu += d * (nb / nn);
  m2 += qb + d * d * (n * nb / nn);
  n = nn;
}

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
  for (int t = t0; t < t1; ++t) {
    const long long left = (long long)n_rows - (long long)t * 32;
    if (left <= 0) break;
    chan_merge(n, mu, m2, left < 32 ? (double)left : 32.0, (double)part[((long long)t * 2) * C + col],
               (double)part[((long long)t * 2 + 1) * C + col]);
  }
  sh[0][seg][lc] = n; sh[1][seg][lc] = mu; sh[2][seg][lc] = m2;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < NSEG; ++s) chan_merge(n, mu, m2, sh[0][s][lc], sh[1][s][lc], sh[2][s][lc]);
  const double var = m2 / n;
  mean[col] = (float)mu;
  invstd[col] = (float)(1.0 / sqrt(var + (double)eps));
  if (rmean) rmean[col] = (float)((1.0 - (double)momentum) * (double)rmean[col] + (double)momentum * mu);
  if (rvar) rvar[col] = (float)((1.0 - (double)momentum) * (double)rvar[col] + (double)momentum * (m2 / (n - 1.0)));
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

// sums of the chunks' partials in a fixed order (32 columns x NSEG segments, as rows_fc_stats_kernel).
// nq == 2: q0 = sum g' -> dbeta, coef[0]; q1 = sum g' xhat -> dgamma, coef[1].  nq == 1: q0 = sum dz -> dbias (out0).
__global__ __launch_bounds__(32 * NSEG) void rows_fc_bwd_sums_kernel(const double* __restrict__ part, int n_chunks, int nq, int C,
                                                               long long n_rows, float* __restrict__ out0, float* __restrict__ out1,
                                                               float* __restrict__ coef) {
  __shared__ double sh[2][NSEG][32];
  const int lc = threadIdx.x & 31, seg = threadIdx.x >> 5, col = blockIdx.x * 32 + lc;
  const int per = (n_chunks + NSEG - 1) / NSEG;
  const int t0 = seg * per, t1 = min(n_chunks, t0 + per);
  double s[2] = {0.0, 0.0};
  for (int t = t0; t < t1; ++t)
    for (int q = 0; q < nq; ++q) s[q] += part[((long long)t * nq + q) * C + col];
  sh[0][seg][lc] = s[0]; sh[1][seg][lc] = s[1];
  __syncthreads();
  if (seg != 0) return;
  for (int k = 1; k < NSEG; ++k) { s[0] += sh[0][k][lc]; s[1] += sh[1][k][lc]; }
  if (nq == 2) {
    if (out0) out0[col] = (float)s[1];                                // dgamma
    if (out1) out1[col] = (float)s[0];                                // dbeta
    if (coef) { coef[col] = (float)(s[0] / (double)n_rows); coef[C + col] = (float)(s[1] / (double)n_rows); }
  } else if (out0) {
    out0[col] = (float)s[0];
  }
}

// dw[co][ci] = sum_n dz[n][co] x[n][ci] over the rows of one split-K chunk; see the file header
template <int TA, int MODE>
__global__ __launch_bounds__(256) void rows_fc_wgrad_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ x, int ldx,
                                                            float* __restrict__ out, long long n_rows, int c_out, int c_in, int chunk) {
  constexpr int TB = 2;
  __shared__ float red[TA * TB * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 32 * TA;
  const int nbv = (c_in - ci0) >= 64 ? 2 : 1;                         // column blocks of x inside c_in (c_in % 32 == 0)
  const int quarter = chunk >> 2;                                     // chunk % 64 == 0
  const long long rb = (long long)blockIdx.z * chunk + (long long)wave * quarter;
  const long long left = n_rows - rb;
  const csn_rsrc_t zr = csn_make_rsrc(dz + rb * ldz, left > 0 ? ((left - 1) * ldz + c_out) * 4LL : 0LL);
  const csn_rsrc_t xr = csn_make_rsrc(x + rb * ldx, left > 0 ? ((left - 1) * ldx + c_in) * 4LL : 0LL);
  // contraction step e of a lane: row 8 h + e (16-bit: 8 consecutive k per lane) or 2 e + h (fp32: one k per lane and instruction)
  const int row_l = MODE == 0 ? h : 8 * h;
  constexpr int ROW_E = MODE == 0 ? 2 : 1;

  f32x16 acc[TA][TB];
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ta][tb][r] = 0.f;

  float an[TA][8], bn[TB][8];
  auto load = [&](int rr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + row_l + ROW_E * e;
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) an[ta][e] = csn_bload(zr, (unsigned)((row * ldz + co0 + ta * 32 + li) * 4));
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) bn[tb][e] = tb < nbv ? csn_bload(xr, (unsigned)((row * ldx + ci0 + tb * 32 + li) * 4)) : 0.f;
    }
  };
  const int n_steps = left <= 0 ? 0 : (int)((left < quarter ? left : quarter) + 15) / 16;
  if (n_steps > 0) load(0);
  for (int st = 0; st < n_steps; ++st) {
    float af[TA][8], bf[TB][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) af[ta][e] = an[ta][e];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) bf[tb][e] = bn[tb][e];
    }
    if (st + 1 < n_steps) load((st + 1) * 16);
    if constexpr (MODE == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int ta = 0; ta < TA; ++ta)
#pragma unroll
          for (int tb = 0; tb < TB; ++tb)
            if (tb < nbv) acc[ta][tb] = csn_mfma(af[ta][e], bf[tb][e], acc[ta][tb]);
    } else {
      s16x8 bhi[TB], blo[TB];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          bhi[tb][e] = to16<false>(bf[tb][e]);
          blo[tb][e] = to16<false>(bf[tb][e] - from16<false>(bhi[tb][e]));
        }
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) {
        s16x8 ahi, alo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ahi[e] = to16<false>(af[ta][e]);
          alo[e] = to16<false>(af[ta][e] - from16<false>(ahi[e]));
        }
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
          if (tb < nbv) {
            acc[ta][tb] = mfma32<false>(alo, bhi[tb], acc[ta][tb]);
            acc[ta][tb] = mfma32<false>(ahi, blo[tb], acc[ta][tb]);
            acc[ta][tb] = mfma32<false>(ahi, bhi[tb], acc[ta][tb]);
          }
      }
    }
  }

  // waves 1..3 are added to wave 0 in wave order
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[((ta * TB + tb) * 16 + r) * 64 + l] = acc[ta][tb][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[ta][tb][r] += red[((ta * TB + tb) * 16 + r) * 64 + l];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  float* o = out + (long long)blockIdx.z * c_out * c_in;
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      if (tb >= nbv) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o[(long long)(co0 + ta * 32 + csn_acc_row(r, h)) * c_in + ci0 + tb * 32 + li] = acc[ta][tb][r];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline long long up256(long long b) { return (b + 255) & ~255LL; }
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
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * ((p.M + 127) / 128);
  if (groups > 0x7fffffffLL) return -5;
  const dim3 grid((unsigned)groups), block(256);
  if (mode == 0) hipLaunchKernelGGL((rows_gemm_kernel<NB, 0, B_KN>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((rows_gemm_kernel<NB, 1, B_KN>), grid, block, 0, st, p);
  return (int)hipGetLastError();
}

// forward products: the wave owns every column up to 128, two column groups at 256
int launch_fwd_gemm(const RowsGemmP& p, int mode, hipStream_t st) {
  switch (p.J) {
    case 32: return launch_gemm_nb<1, false>(p, mode, st);
    case 64: return launch_gemm_nb<2, false>(p, mode, st);
    case 96: return launch_gemm_nb<3, false>(p, mode, st);
    default: return launch_gemm_nb<4, false>(p, mode, st);
  }
}

template <int TA>
int launch_wgrad_ta(const float* dz, const float* x, int ldx, float* out, long long n_rows, int c_in, int c_out, int splits, int chunk,
                    int mode, hipStream_t st) {
  const dim3 grid((unsigned)((c_in + 63) / 64), (unsigned)(c_out / (32 * TA)), (unsigned)splits), block(256);
  if (mode == 0) hipLaunchKernelGGL((rows_fc_wgrad_kernel<TA, 0>), grid, block, 0, st, dz, c_out, x, ldx, out, n_rows, c_out, c_in, chunk);
  else hipLaunchKernelGGL((rows_fc_wgrad_kernel<TA, 1>), grid, block, 0, st, dz, c_out, x, ldx, out, n_rows, c_out, c_in, chunk);
  return (int)hipGetLastError();
}

}  // namespace

long long csn_rows_fc_ws_bytes(long long n_rows, int c_in, int c_out, int training, int backward) {
  return ws_layout(n_rows, c_in, c_out, training, backward).total;
}

int csn_launch_rows_fc_fwd(const CsnRowsFcArgs& a, int mode, hipStream_t st) {
  mode = mode != 0;
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
  mode = mode != 0;
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
  hipLaunchKernelGGL(rows_fc_bwd_sums_kernel, dim3(a.c_out / 32), dim3(32 * NSEG), 0, st, part, n_chunks, 2, a.c_out, (long long)a.n_rows,
                     a.dgamma, a.dbeta, coef);
  if (const int e = (int)hipGetLastError()) return e;
  if (!a.dx && !a.dw && !a.dbias) return 0;
  if (!a.dbias) b.part = nullptr;
  hipLaunchKernelGGL(rows_fc_bwd_kernel<2>, dim3(n_chunks), dim3(256), 0, st, b);
  if (const int e = (int)hipGetLastError()) return e;
  if (a.dbias) {
    hipLaunchKernelGGL(rows_fc_bwd_sums_kernel, dim3(a.c_out / 32), dim3(32 * NSEG), 0, st, part, n_chunks, 1, a.c_out, (long long)a.n_rows,
                       a.dbias, (float*)nullptr, (float*)nullptr);
    if (const int e = (int)hipGetLastError()) return e;
  }
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
    int e;
    switch (wgrad_ta(a.c_out)) {
      case 1: e = launch_wgrad_ta<1>(dz, a.x, a.ld_x, out, a.n_rows, a.c_in, a.c_out, splits, chunk, mode, st); break;
      case 2: e = launch_wgrad_ta<2>(dz, a.x, a.ld_x, out, a.n_rows, a.c_in, a.c_out, splits, chunk, mode, st); break;
      case 3: e = launch_wgrad_ta<3>(dz, a.x, a.ld_x, out, a.n_rows, a.c_in, a.c_out, splits, chunk, mode, st); break;
      default: e = launch_wgrad_ta<4>(dz, a.x, a.ld_x, out, a.n_rows, a.c_in, a.c_out, splits, chunk, mode, st); break;
    }
    if (e) return e;
    if (splits > 1) return csn_launch_slab_reduce(out, a.dw, splits, (long long)a.c_out * a.c_in, 1.f, 0, st);
  }
  return 0;
}
