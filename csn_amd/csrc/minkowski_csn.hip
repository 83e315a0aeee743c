// The ragged (per-shape-length) parts of the MinkowskiNet cross-shape head (MinkowskiNet/models/hrnet.py:359-423) around
// the varlen attention: pooled SSA descriptors, the compatibility-weighted mix and their backward.
//
// The attention layer leaves every evaluation e as a channel-major, pre-affine map xhat[e][c][0..ld) (the LayerNorm affine
// gamma / beta is applied here, never materialised per evaluation).  Evaluation e has counts[e] real points; the varlen
// attention ran it with round-up-4(counts[e]) queries, so the points [counts[e], round-up-4) hold REAL, non-zero values
// (attention of a zero query is the mean of V).  Every kernel here uses the exact count: those points enter no sum and
// their gradient is written as zero.  Every point of xhat up to ld must be FINITE all the same: the mix backward forms
// 0 * xhat for the points between a shape's count and the end of its last 64-point tile (an inf or nan there would reach
// rowdot).  The attention keeps that promise: the context of a padding query is zero, and fc + LayerNorm of a zero row is a
// finite row (minkowski_attention.py, _CrossMHA.forward).
//   pool     pooled[e][c] = gamma[c] mean_{n < counts[e]} xhat[e][c][n] + beta[c]                      (hrnet.py:380-381, 388-389)
//   mix fwd   out[off[b] + n][c] = sum_j comp[b][j] (gamma[c] xhat[ev(b,j)][c][n] + beta[c])            (hrnet.py:397-411)
//             written POINT-MAJOR into the caller's row (the csa half of the output layer's input: the concatenation of
//             hrnet.py:423 costs nothing)
//   mix bwd   dxhat[ev(b,j)][c][n] = comp[b][j] gamma[c] dout[off[b] + n][c]; per-(shape, slot, channel) dot products and
//             per-(shape, channel) sums from which d comp, d gamma and d beta follow
//   pool bwd  dxhat[e][c][n] (+)= gamma[c] dpooled[e][c] / counts[e]
// ev(b, 0) = b (the shape's own SSA), ev(b, j > 0) = cross_first + (j - 1) n_shapes + b (MHA(q_b, k_{j,b}, k_{j,b})).
// Every sum accumulates in fp64 in a fixed order (bitwise reproducible).
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int TP = 64;                    // points per mix tile
constexpr int TC = 64;                    // channels per mix tile

CSN_DEVINL double block_sum256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

CSN_DEVINL int mix_eval(int b, int j, int B, int cross_first) { return j == 0 ? b : cross_first + (j - 1) * B + b; }

// one work-group per (evaluation, channel) row
__global__ __launch_bounds__(256) void csn_ragged_pool_kernel(const float* __restrict__ xhat, long long eval_stride, int ld,
                                                              const int* __restrict__ counts, int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ pooled,
                                                              float* __restrict__ mean) {
  __shared__ double red[4];
  const int e = blockIdx.x / C, c = blockIdx.x % C;
  const int n = counts[e];
  const float* __restrict__ p = xhat + (long long)e * eval_stride + (long long)c * ld;
  double s = 0.0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {           // i + 3 < ld: ld % 4 == 0 and i < n <= ld
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + i);
    s += ((double)v.x + (i + 1 < n ? (double)v.y : 0.0)) + ((i + 2 < n ? (double)v.z : 0.0) + (i + 3 < n ? (double)v.w : 0.0));
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) {
    const double m = s / (double)n;
    pooled[(long long)e * C + c] = (float)((double)gamma[c] * m + (double)beta[c]);
    if (mean) mean[(long long)e * C + c] = (float)m;
  }
}

// dxhat[e][c][n] = (accumulate ? dxhat : 0) + (n < counts[e] ? gamma[c] dpooled[e][c] / counts[e] : 0), n < ld
__global__ __launch_bounds__(256) void csn_ragged_pool_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ gamma,
                                                                  const int* __restrict__ counts, int C, float* __restrict__ dxhat,
                                                                  long long eval_stride, int ld, int accumulate) {
  const int e = blockIdx.z, c = blockIdx.y;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= ld) return;
  const int n = counts[e];
  const float g = (float)((double)gamma[c] * (double)dpooled[(long long)e * C + c] / (double)n);
  float* __restrict__ p = dxhat + (long long)e * eval_stride + (long long)c * ld + i;
  f32x4 v = accumulate ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
  if (i < n) v.x += g;
  if (i + 1 < n) v.y += g;
  if (i + 2 < n) v.z += g;
  if (i + 3 < n) v.w += g;
  *reinterpret_cast<f32x4*>(p) = v;
}

// a (TP points x TC channels) tile of shape b: thread t owns channel t / 4 and the 16 points 16 (t % 4) .. of the tile
__global__ __launch_bounds__(256) void csn_ragged_mix_fwd_kernel(const float* __restrict__ xhat, long long eval_stride, int ld,
                                                                 int cross_first, const int* __restrict__ offsets, int B, int K1, int C,
                                                                 const float* __restrict__ comp, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ out,
                                                                 long long ld_out) {
  __shared__ float tile[TP][TC + 1];
  const int b = blockIdx.z, n0 = blockIdx.x * TP, c0 = blockIdx.y * TC;
  const int row0 = offsets[b], nb = offsets[b + 1] - row0;
  if (n0 >= nb) return;                                        // a short shape costs its own size
  const int t = threadIdx.x, cl = t >> 2, nl = (t & 3) * 16, c = c0 + cl;
  float acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  float csum = 0.f;
  if (c < C) {
    for (int j = 0; j < K1; ++j) {
      const float w = comp[b * K1 + j];
      csum += w;
      const float* __restrict__ p = xhat + (long long)mix_eval(b, j, B, cross_first) * eval_stride + (long long)c * ld + n0 + nl;
#pragma unroll
      for (int q = 0; q < 16; q += 4) {
        if (n0 + nl + q < ld) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(p + q);
          acc[q] = fmaf(w, v.x, acc[q]); acc[q + 1] = fmaf(w, v.y, acc[q + 1]);
          acc[q + 2] = fmaf(w, v.z, acc[q + 2]); acc[q + 3] = fmaf(w, v.w, acc[q + 3]);
        }
      }
    }
    const float g = gamma[c], bt = beta[c] * csum;
#pragma unroll
    for (int q = 0; q < 16; ++q) tile[nl + q][cl] = fmaf(g, acc[q], bt);
  }
  __syncthreads();
  // point-major write: thread t owns point t / 4 and the 16 channels 16 (t % 4) ..
  const int pn = t >> 2, pc = (t & 3) * 16;
  if (n0 + pn >= nb) return;
  float* __restrict__ o = out + (long long)(row0 + n0 + pn) * ld_out + c0 + pc;
#pragma unroll
  for (int q = 0; q < 16; q += 4)
    if (c0 + pc + q < C) {
      const f32x4 v = {tile[pn][pc + q], tile[pn][pc + q + 1], tile[pn][pc + q + 2], tile[pn][pc + q + 3]};
      *reinterpret_cast<f32x4*>(o + q) = v;
    }
}

// backward of the mix.  ws[b][j][tile][c] (j < K1: sum_n dout xhat_ev(b,j); j == K1: sum_n dout) per 64-point tile, fp64
__global__ __launch_bounds__(256) void csn_ragged_mix_bwd_kernel(const float* __restrict__ dout, long long ld_dout,
                                                                 const float* __restrict__ xhat, long long eval_stride, int ld,
                                                                 int cross_first, const int* __restrict__ offsets, int B, int K1, int C,
                                                                 const float* __restrict__ comp, const float* __restrict__ gamma,
                                                                 float* __restrict__ dxhat, double* __restrict__ ws, int tiles) {
  __shared__ float tile[TP][TC + 1];
  const int b = blockIdx.z, n0 = blockIdx.x * TP, c0 = blockIdx.y * TC;
  const int row0 = offsets[b], nb = offsets[b + 1] - row0;
  const int t = threadIdx.x;
  // stage the gradient tile (point-major rows, zero beyond the shape's points)
  {
    const int pn = t >> 2, pc = (t & 3) * 16;
    const bool on = n0 + pn < nb;
    const float* __restrict__ src = dout + (long long)(row0 + n0 + pn) * ld_dout + c0 + pc;
#pragma unroll
    for (int q = 0; q < 16; q += 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (on && c0 + pc + q < C) v = *reinterpret_cast<const f32x4*>(src + q);
      tile[pn][pc + q] = v.x; tile[pn][pc + q + 1] = v.y; tile[pn][pc + q + 2] = v.z; tile[pn][pc + q + 3] = v.w;
    }
  }
  __syncthreads();
  const int cl = t >> 2, nl = (t & 3) * 16, c = c0 + cl;
  if (c >= C) return;                                          // (no barrier follows)
  float d[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) d[q] = tile[nl + q][cl];
  const bool live = n0 < nb;                                   // tiles past the shape only write zeros
  const float g = gamma[c];
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) s += (double)d[q];
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (live && (t & 3) == 0) ws[(((long long)b * (K1 + 1) + K1) * tiles + blockIdx.x) * C + c] = s;
  for (int j = 0; j < K1; ++j) {
    const long long base = (long long)mix_eval(b, j, B, cross_first) * eval_stride + (long long)c * ld + n0 + nl;
    const float w = comp[b * K1 + j] * g;
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < 16; q += 4) {
      if (n0 + nl + q < ld) {
        if (live) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(xhat + base + q);
          // d is zero beyond the shape's points: the real-but-padding xhat there adds nothing
          dot += ((double)d[q] * (double)x.x + (double)d[q + 1] * (double)x.y) +
                 ((double)d[q + 2] * (double)x.z + (double)d[q + 3] * (double)x.w);
        }
        const f32x4 v = {w * d[q], w * d[q + 1], w * d[q + 2], w * d[q + 3]};
        *reinterpret_cast<f32x4*>(dxhat + base + q) = v;
      }
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    if (live && (t & 3) == 0) ws[(((long long)b * (K1 + 1) + j) * tiles + blockIdx.x) * C + c] = dot;
  }
}

// rowdot[b][j][c] / rowsum[b][c] = the tile partials of the shape's own tiles, added in tile order
__global__ __launch_bounds__(256) void csn_ragged_mix_sums_kernel(const double* __restrict__ ws, const int* __restrict__ offsets,
                                                                  int K1, int C, int tiles, double* __restrict__ rowdot,
                                                                  double* __restrict__ rowsum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int bj = blockIdx.y, b = bj / (K1 + 1), j = bj % (K1 + 1);
  if (c >= C) return;
  const int nt = (offsets[b + 1] - offsets[b] + TP - 1) / TP;
  const double* __restrict__ p = ws + (long long)bj * tiles * C + c;
  double s = 0.0;
  for (int i = 0; i < nt; ++i) s += p[(long long)i * C];
  if (j < K1) rowdot[((long long)b * K1 + j) * C + c] = s;
  else rowsum[(long long)b * C + c] = s;
}

}  // namespace

int csn_ragged_mix_tiles(int max_points) { return (max_points + TP - 1) / TP; }

int csn_launch_ragged_pool_f32(const float* xhat, long long eval_stride, int ld, const int* counts, int E, int C, const float* gamma,
                               const float* beta, float* pooled, float* mean, hipStream_t st) {
  hipLaunchKernelGGL(csn_ragged_pool_kernel, dim3((unsigned)E * C), dim3(256), 0, st, xhat, eval_stride, ld, counts, C, gamma, beta,
                     pooled, mean);
  return (int)hipGetLastError();
}

int csn_launch_ragged_pool_bwd_f32(const float* dpooled, const float* gamma, const int* counts, int E, int C, float* dxhat,
                                   long long eval_stride, int ld, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(csn_ragged_pool_bwd_kernel, dim3((unsigned)((ld + 1023) / 1024), C, E), dim3(256), 0, st, dpooled, gamma, counts,
                     C, dxhat, eval_stride, ld, accumulate);
  return (int)hipGetLastError();
}

int csn_launch_ragged_mix_fwd_f32(const float* xhat, long long eval_stride, int ld, int cross_first, const int* offsets, int B,
                                  int K1, int C, int max_points, const float* comp, const float* gamma, const float* beta, float* out,
                                  long long ld_out, hipStream_t st) {
  hipLaunchKernelGGL(csn_ragged_mix_fwd_kernel, dim3((unsigned)csn_ragged_mix_tiles(max_points), (C + TC - 1) / TC, B), dim3(256), 0,
                     st, xhat, eval_stride, ld, cross_first, offsets, B, K1, C, comp, gamma, beta, out, ld_out);
  return (int)hipGetLastError();
}

int csn_launch_ragged_mix_bwd_f32(const float* dout, long long ld_dout, const float* xhat, long long eval_stride, int ld,
                                  int cross_first, const int* offsets, int B, int K1, int C, const float* comp, const float* gamma,
                                  float* dxhat, double* rowdot, double* rowsum, double* ws, hipStream_t st) {
  const int tiles = csn_ragged_mix_tiles(ld);                  // every point of every mixed map is written (zeros past the shape)
  hipLaunchKernelGGL(csn_ragged_mix_bwd_kernel, dim3((unsigned)tiles, (C + TC - 1) / TC, B), dim3(256), 0, st, dout, ld_dout, xhat,
                     eval_stride, ld, cross_first, offsets, B, K1, C, comp, gamma, dxhat, ws, tiles);
  hipLaunchKernelGGL(csn_ragged_mix_sums_kernel, dim3((unsigned)((C + 255) / 256), B * (K1 + 1)), dim3(256), 0, st, ws, offsets, K1,
                     C, tiles, rowdot, rowsum);
  return (int)hipGetLastError();
}
