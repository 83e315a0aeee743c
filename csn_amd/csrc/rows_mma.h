// The bodies that the row products of the MinkowskiNet side share, stated once: rows_gemm / rows_fc_wgrad (rows_fc.hip, dense rows),
// sconv_gemm / sconv_wgrad (sparse_conv.hip, rows looked up in a kernel map) and the BatchNorm statistics merges (rows_fc.hip,
// rows_bn_act.hip).  A kernel keeps where its rows come from, its pipeline order and its launch rule; what it does with a
// staged tile is here.
//
//   row product      a wave owns 32 rows x NB * 32 columns; a lane owns one row and 4 (fp32) / 8 (16-bit) consecutive k of every
//                    32-k step (a_kofs); B — [J][K] or [K][J] (B_KN) — is staged through LDS once per work-group (load_b,
//                    store_b); mma_step contracts one step; store_tile adds the bias, stores the wave's rows and forms their
//                    (mean, M2) from the accumulators; store_tile_bn stores act(acc * s + t + r) instead (inference).
//                    mma_step_a16 is the single-product step on A fragments that ARE 16-bit (the 16-bit maps of
//                    sparse_conv_maps16.hip and octant_conv_maps16.hip: two 16-byte loads per step, no conversion).
//   octant tiles     octant_span: the (octant, range) of `order` a work-group or a chunk owns (octant_conv.hip,
//                    octant_conv_maps16.hip, octant_conv_stats.hip).
//   weight gradient  both operands are k-major (the contraction runs over the rows): a lane holds 8 rows of one column per 16-row
//                    step (wgrad_row) and splits them in registers (wgrad_step); the four waves of a work-group contract a
//                    quarter of its row chunk each and are added through LDS in wave order (wgrad_reduce_store).
//   MODE              0 fp32, 1 bf16x3 (hi / lo split in registers, three products), 2 bf16 / 3 fp16: ONE product of operands
//                    rounded once to 16 bits (to16x4: nearest even) — A in registers, B when it is stored to LDS, so the tile
//                    holds shorts and a lane's B fragment is one 16-byte read.
//   statistics       chan_merge / chan_walk / bn_finish: [tile][2][C] (mean, M2) partials of 32-row tiles -> mean, invstd,
//                    running statistics, in fp64.  chan_walk_counts: the same over tiles that carry their own row counts
//                    (octant_conv_stats.hip).
// Every reduction has a fixed order.
#pragma once
#include <type_traits>

#include "csn_kernels.h"

namespace rows_mma {
using namespace csn_mode;

constexpr int BS_PITCH = 36;          // floats per LDS row of the B tile: 32 k + 4 (16-byte reads of 16 lanes hit 16 x 4 distinct banks)
constexpr int BS16_PITCH = 40;        // shorts per row of the single-product tile: 32 k + 8 (20 li mod 64 is a distinct multiple of 4 dwords
                                      // over each 16-lane group of a 16-byte read)
template <int MODE> using bs_t = std::conditional_t<(MODE >= 2), short, float>;
template <int MODE> constexpr int bs_pitch = MODE >= 2 ? BS16_PITCH : BS_PITCH;
constexpr int WG_TB = 2;              // 32-column blocks of the weight gradient's second operand per work-group

// k of a lane's g-th 16-byte A read inside a 32-k step, before its half-wave offset (4 h fp32, 8 h 16-bit):
// fp32: k = 8 g + 4 h + t; 16-bit: k = 16 (g / 2) + 8 h + 4 (g % 2) + t
template <int MODE>
__device__ __forceinline__ constexpr int a_kofs(int g) { return MODE == 0 ? 8 * g : 16 * (g >> 1) + 4 * (g & 1); }

// 32 k x NB * 32 columns of B from column j0 and contraction index k0 into registers (columns past J read as zero) ...
template <int NB, bool B_KN>
__device__ __forceinline__ void load_b(f32x4 (&bn)[NB], const float* b, int ldb, int k0, int j0, int J, int tid) {
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int idx = tid + 256 * u;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!B_KN) {
      const int j = idx >> 3, kq = idx & 7;
      if (j0 + j < J) v = *reinterpret_cast<const f32x4*>(b + (long long)(j0 + j) * ldb + k0 + 4 * kq);
    } else {
      const int k = idx / (NB * 8), jq = idx % (NB * 8);
      if (j0 + 4 * jq < J) v = *reinterpret_cast<const f32x4*>(b + (long long)(k0 + k) * ldb + j0 + 4 * jq);
    }
    bn[u] = v;
  }
}

// ... and from there into the LDS tile Bs[column][bs_pitch]: floats, or (single product) the values rounded to 16 bits
template <int NB, bool B_KN, int MODE>
__device__ __forceinline__ void store_b(bs_t<MODE>* Bs, const f32x4 (&bn)[NB], int tid) {
  constexpr int P = bs_pitch<MODE>;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int idx = tid + 256 * u;
    if constexpr (!B_KN) {
      const int j = idx >> 3, kq = idx & 7;
      if constexpr (MODE >= 2) *reinterpret_cast<s16x4*>(&Bs[j * P + 4 * kq]) = to16x4<MODE == 3>(bn[u]);
      else *reinterpret_cast<f32x4*>(&Bs[j * P + 4 * kq]) = bn[u];
    } else {
      const int k = idx / (NB * 8), jq = idx % (NB * 8);
      if constexpr (MODE >= 2) {
        const s16x4 v = to16x4<MODE == 3>(bn[u]);
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(4 * jq + e) * P + k] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(4 * jq + e) * P + k] = bn[u][e];
      }
    }
  }
}

// one 32-k step: the lane's A reads af[g] (a_kofs) against the staged tile
template <int NB, int MODE>
__device__ __forceinline__ void mma_step(f32x16 (&acc)[NB], const f32x4 (&af)[4], const bs_t<MODE>* Bs, int li, int h) {
  if constexpr (MODE >= 2) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const s16x8 a = join8(to16x4<MODE == 3>(af[2 * s2]), to16x4<MODE == 3>(af[2 * s2 + 1]));
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = mfma32<MODE == 3>(a, *reinterpret_cast<const s16x8*>(&Bs[(nb * 32 + li) * BS16_PITCH + 16 * s2 + 8 * h]), acc[nb]);
    }
  } else if constexpr (MODE == 0) {
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

// one 32-k step on 16-bit A: the lane's two fragments against the staged tile, in mma_step's order (half step, column block)
template <int NB, bool H16>
__device__ __forceinline__ void mma_step_a16(f32x16 (&acc)[NB], const f32x4 (&af)[2], const short* Bs, int li, int h) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const s16x8 a = __builtin_bit_cast(s16x8, af[s2]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = mfma32<H16>(a, *reinterpret_cast<const s16x8*>(&Bs[(nb * 32 + li) * BS16_PITCH + 16 * s2 + 8 * h]), acc[nb]);
  }
}

// One 32 x 32 accumulator block of a wave (column `col` of rows row_w .. row_w + 31, of which the first cnt exist): z = acc + bv
// is stored to c; with `stats` the (mean, M2) of the cnt rows go to part[tile][2][J] — two passes over the registers (no
// cancellation); the stored values are the same bits either way.  A store's address is a wave-uniform row address (scalar
// registers) plus one lane offset: sixteen per-lane 64-bit addresses per block would cost the wider instances a wave per SIMD.
__device__ __forceinline__ void store_tile(f32x16& acc, float bv, float* c, int ldc, long long row_w, int cnt, int col, int h, bool stats,
                                           float* part, long long tile, int J) {
  float* cw = c + row_w * ldc;
  const int lane = 4 * h * ldc + col;
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rr = csn_acc_row(r, h);
    const float v = acc[r] + bv;
    acc[r] = v;
    if (rr < cnt) { (cw + csn_acc_row(r, 0) * ldc)[lane] = v; sum += v; }
  }
  if (stats) {
    sum += csn_xhalf(sum);
    const float mu = cnt > 0 ? sum / (float)cnt : 0.f;
    float m2 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[r] - mu;
      if (csn_acc_row(r, h) < cnt) m2 = fmaf(d, d, m2);
    }
    m2 += csn_xhalf(m2);
    if (h == 0) {
      part[(tile * 2) * J + col] = mu;
      part[(tile * 2 + 1) * J + col] = m2;
    }
  }
}

// The same block through an inference epilogue: y = act(acc * s + t + r) with the lane's column constants s, t (a BatchNorm on its
// running statistics), an optional residual map r (pitch ldr) and act = ReLU or the identity; nothing but y is written.  r is read
// through the same address form as the store, and each element is read and then written by the same lane: r may be c itself (with
// ldr == ldc), which is how a sum over branches accumulates in one buffer.
__device__ __forceinline__ void store_tile_bn(const f32x16& acc, float s, float t, const float* r, int ldr, bool relu, float* c, int ldc,
                                              long long row_w, int cnt, int col, int h) {
  float* cw = c + row_w * ldc;
  const int lane = 4 * h * ldc + col;
  const float* rw = r ? r + row_w * ldr : nullptr;
  const int lane_r = 4 * h * ldr + col;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    if (csn_acc_row(q, h) >= cnt) continue;
    float v = fmaf(acc[q], s, t);
    if (rw) v += (rw + csn_acc_row(q, 0) * ldr)[lane_r];
    (cw + csn_acc_row(q, 0) * ldc)[lane] = relu ? fmaxf(0.f, v) : v;
  }
}

// ---- octant tiles (octant_conv.hip, octant_conv_maps16.hip) ---------------------------------------------------------------
// The span of `order` that slot t owns when every segment is cut into spans of `span` entries: its octant k and [lo, hi).
// false: the slot has none.  Wave-uniform (9 scalar reads).
__device__ __forceinline__ bool octant_span(const int* __restrict__ seg, int n, int t, int span, int& k, int& lo, int& hi) {
  int s0 = min(max(seg[0], 0), n);
  for (int kk = 0; kk < 8; ++kk) {
    const int s1 = min(max(seg[kk + 1], s0), n);
    const int cnt = (s1 - s0 + span - 1) / span;
    if (t < cnt) {
      k = kk; lo = s0 + t * span; hi = min(lo + span, s1);
      return true;
    }
    t -= cnt;
    s0 = s1;
  }
  return false;
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
// row of a lane's contraction step e inside a 16-row step: 8 h + e (16-bit: 8 consecutive k per lane) or 2 e + h (fp32: one k
// per lane and instruction)
template <int MODE>
__device__ __forceinline__ constexpr int wgrad_row(int h, int e) { return MODE == 0 ? h + 2 * e : 8 * h + e; }

// 16-row steps of a wave's quarter of the chunk, `left` rows from its first to the end of the map
__device__ __forceinline__ int wgrad_steps(long long left, int quarter) {
  return left <= 0 ? 0 : (int)((left < quarter ? left : quarter) + 15) / 16;
}

// 8 floats rounded to 16 bits (nearest even) as one matrix-core fragment
template <bool H16>
__device__ __forceinline__ s16x8 pack8(const float (&v)[8]) {
  return join8(to16x4<H16>(f32x4{v[0], v[1], v[2], v[3]}), to16x4<H16>(f32x4{v[4], v[5], v[6], v[7]}));
}

// one 16-row step: acc[ta][tb] += af[ta]^T bf[tb] over the lane's 8 rows, for the nbv column blocks that exist.  SPLIT_ALL: bf16x3
// splits an absent block of bf too (never read) instead of branching round it: the gathered kernel is 8 % faster so, the dense one
// a wave per SIMD poorer at TA 2
template <int TA, int MODE, bool SPLIT_ALL>
__device__ __forceinline__ void wgrad_step(f32x16 (&acc)[TA][WG_TB], const float (&af)[TA][8], const float (&bf)[WG_TB][8], int nbv) {
  if constexpr (MODE == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < WG_TB; ++tb)
          if (tb < nbv) acc[ta][tb] = csn_mfma(af[ta][e], bf[tb][e], acc[ta][tb]);
  } else if constexpr (MODE >= 2) {
    // one conversion of the lane's 8 rows per operand (an absent block of bf is converted too: it is never read), one product
    s16x8 b16[WG_TB];
#pragma unroll
    for (int tb = 0; tb < WG_TB; ++tb) b16[tb] = pack8<MODE == 3>(bf[tb]);
#pragma unroll
    for (int ta = 0; ta < TA; ++ta) {
      const s16x8 a16 = pack8<MODE == 3>(af[ta]);
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb)
        if (tb < nbv) acc[ta][tb] = mfma32<MODE == 3>(a16, b16[tb], acc[ta][tb]);
    }
  } else {
    s16x8 bhi[WG_TB], blo[WG_TB];
#pragma unroll
    for (int tb = 0; tb < WG_TB; ++tb)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (!SPLIT_ALL && tb >= nbv) continue;
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
      for (int tb = 0; tb < WG_TB; ++tb)
        if (tb < nbv) {
          acc[ta][tb] = mfma32<false>(alo, bhi[tb], acc[ta][tb]);
          acc[ta][tb] = mfma32<false>(ahi, blo[tb], acc[ta][tb]);
          acc[ta][tb] = mfma32<false>(ahi, bhi[tb], acc[ta][tb]);
        }
    }
  }
}

// the single-product step (MODE 2) on A fragments that ARE bf16 (train_maps16.hip: x is a bf16 map): bf converted as there, the
// same instructions in the same (ta, tb) order
template <int TA>
__device__ __forceinline__ void wgrad_step_a16(f32x16 (&acc)[TA][WG_TB], const s16x8 (&a16)[TA], const float (&bf)[WG_TB][8], int nbv) {
  s16x8 b16[WG_TB];
#pragma unroll
  for (int tb = 0; tb < WG_TB; ++tb) b16[tb] = pack8<false>(bf[tb]);
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < WG_TB; ++tb)
      if (tb < nbv) acc[ta][tb] = mfma32<false>(a16[ta], b16[tb], acc[ta][tb]);
}

// waves 1..3 are added to wave 0 in wave order through red[TA * WG_TB * 16 * 64]; wave 0 stores block (ta, tb) at row
// row0 + 32 ta, column col0 + 32 tb of o (row pitch `pitch`)
template <int TA>
__device__ __forceinline__ void wgrad_reduce_store(f32x16 (&acc)[TA][WG_TB], float* red, float* o, int pitch, int row0, int col0, int nbv,
                                                   int wave, int l) {
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < WG_TB; ++tb)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[((ta * WG_TB + tb) * 16 + r) * 64 + l] = acc[ta][tb][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < WG_TB; ++tb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[ta][tb][r] += red[((ta * WG_TB + tb) * 16 + r) * 64 + l];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  const int li = l & 31, h = l >> 5;
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < WG_TB; ++tb) {
      if (tb >= nbv) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o[(long long)(row0 + ta * 32 + csn_acc_row(r, h)) * pitch + col0 + tb * 32 + li] = acc[ta][tb][r];
    }
}

// ---- BatchNorm statistics from [tile][2][C] (mean, M2) partials of 32-row tiles ----------------------------------------
// Chan's merge of (n, mean, M2) pairs
__device__ __forceinline__ void chan_merge(double& n, double& mu, double& m2, double nb, double mb, double qb) {
  if (nb <= 0.0) return;
  const double nn = n + nb, d = mb - mu;
  mu += d * (nb / nn);
  m2 += qb + d * d * (n * nb / nn);
  n = nn;
}

// tiles t0 .. t1 - 1 of column col merged in tile order; the last tile of the n_rows rows may be short
__device__ __forceinline__ void chan_walk(double& n, double& mu, double& m2, const float* __restrict__ part, int t0, int t1, int n_rows,
                                          int C, int col) {
  for (int t = t0; t < t1; ++t) {
    const long long left = (long long)n_rows - (long long)t * 32;
    if (left <= 0) break;
    chan_merge(n, mu, m2, left < 32 ? (double)left : 32.0, (double)part[((long long)t * 2) * C + col],
               (double)part[((long long)t * 2 + 1) * C + col]);
  }
}

// the same walk over tiles that hold cnt[t] rows each, 0 .. 32 in any order (the octant tiles of octant_conv_stats.hip, cut at the
// segment bounds: a short or empty tile may sit anywhere in the list); an empty tile's partial is not read
__device__ __forceinline__ void chan_walk_counts(double& n, double& mu, double& m2, const float* __restrict__ part,
                                                 const int* __restrict__ cnt, int t0, int t1, int C, int col) {
  for (int t = t0; t < t1; ++t) {
    const int c = cnt[t];
    if (c <= 0) continue;
    chan_merge(n, mu, m2, (double)c, (double)part[((long long)t * 2) * C + col], (double)part[((long long)t * 2 + 1) * C + col]);
  }
}

// mean, invstd (biased variance) and the running statistics (unbiased variance) of one column
__device__ __forceinline__ void bn_finish(double n, double mu, double m2, int col, float eps, float momentum, float* __restrict__ mean,
                                          float* __restrict__ invstd, float* __restrict__ rmean, float* __restrict__ rvar) {
  mean[col] = (float)mu;
  invstd[col] = (float)(1.0 / sqrt(m2 / n + (double)eps));
  if (rmean) rmean[col] = (float)((1.0 - (double)momentum) * (double)rmean[col] + (double)momentum * mu);
  if (rvar) rvar[col] = (float)((1.0 - (double)momentum) * (double)rvar[col] + (double)momentum * (m2 / (n - 1.0)));
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline long long up256(long long b) { return (b + 255) & ~255LL; }

// a row product's grid: one work-group per (128 rows, NB * 32 columns), column groups fastest; k[mode] are the kernel's fp32,
// bf16x3, bf16 and fp16 instances of that NB (the last may be NULL: a backward product has no fp16 form, -1 = CSN_E_ARG)
template <typename P>
int launch_row_product(void (*const (&k)[4])(P), const P& p, int NB, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * ((p.M + 127) / 128);
  if (groups > 0x7fffffffLL) return -5;
  if (mode < 0 || mode > 3 || !k[mode]) return -1;
  hipLaunchKernelGGL(k[mode], dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// f(std::integral_constant<int, n>) for n = 1 .. 3, and 4 for everything above: the NB / TA instance of a launch
template <typename F>
int dispatch4(int n, F&& f) {
  switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

}  // namespace rows_mma
