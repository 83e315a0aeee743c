// Sparse 3D convolution on voxel rows (MinkowskiNet/models/hrnet.py:39-53, 89-111, 233-239; models/modules/resnet_block.py:22-57):
// kernel 3 / 5 at stride 1, kernel 3 at stride 2 and its transposed form are ONE gather-GEMM over a kernel map
// table[KV][n_out] (int32: the source row of output row j at offset k, or -1) — forward and backward.
//
//   sconv_gemm         C[j] = sum_k A[table[k][j]] * B[k] (+ bias).  rows_gemm of rows_fc.hip with a lane's row address looked up
//                      per offset: a lane owns one output row and reads 4 / 8 consecutive channels of its source row through one
//                      buffer descriptor over the whole source map; a -1 entry (and a row past the end) gives the lane CSN_OOB, so
//                      it reads zeros — no lane mask around the matrix instructions.  The contraction runs over (offset,
//                      32-channel step); each W[k] step is staged through LDS once per work-group.  An offset at which no row of
//                      the work-group's 128-row tile has a neighbour is dropped from the work-group's offset list before the loop
//                      (wave ballots, merged through LDS: uniform over the work-group).  Forward: A = x, table = fwd, B[k] =
//                      W[k] ([c_in][c_out], B_KN).  dx: A = dy, table = bwd, B[k] = W[k]^T (the same memory read [J][K]).
//                      Every output row is written by exactly one wave.  With a partials pointer the epilogue also forms the
//                      (mean, M2) of each wave's <= 32 rows from the accumulators (the BatchNorm statistics of the backbone's
//                      convolutions, csn_sparse_conv_stats_fwd_f32); the stored values are the same bits either way.
//   sconv_wgrad        dW[k][ci][co] = sum_j x[fwd[k][j]][ci] dy[j][co] over the output rows of one split-K chunk: rows_fc_wgrad
//                      with one gathered operand (a lane's 8 contraction steps are 8 looked-up rows of one column: a half wave
//                      reads one contiguous 128-byte run per row).  A 16-row step in which the wave finds no neighbour is skipped
//                      (wave ballot).  The four waves contract a quarter of the chunk each and are added through LDS in wave
//                      order; the chunks are slabs added in order by csn_launch_slab_reduce.
//   sconv_colsum / sconv_colsum_merge   dbias = sum_j dy[j]: fp64 sums of 64-row chunks, added in chunk order.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "csn_kernels.h"

namespace {
using namespace csn_mode;

constexpr int BS_PITCH = 36;          // floats per LDS row of the B tile (rows_fc.hip)
constexpr int MAX_KV = 125;
// Work-groups a launch should offer before it is split finer: the CUs of an MI355X (one work-group per CU).  It only chooses
// between forms of one product (the column blocks a wave owns, the split-K chunks); it changes no sum.
constexpr int TARGET_GROUPS = 256;

struct SconvGemmP {
  const float* a; int lda; int n_src;  // A[n_src][lda]: the gathered map
  const int* table;                    // [KV][M]
  int rev;                             // 1: offset k reads table[KV - 1 - k] (stride 1: bwd[k] = fwd[KV - 1 - k], no second table)
  const float* b;                      // W[KV][c_in][c_out]
  int c_in, c_out;
  float* c; int ldc;                   // C[M][J]
  int M, K, J, KV;
  const float* bias;
  float* part;                         // non-NULL: the (mean, M2) of each wave's rows, [tile][2][J], tile = 32 rows (rows_fc.hip)
};

template <int NB, int MODE, bool B_KN>
__global__ __launch_bounds__(256) void sconv_gemm_kernel(const SconvGemmP p) {
  __shared__ __attribute__((aligned(16))) float Bs[NB * 32 * BS_PITCH];
  __shared__ int s_flag[MAX_KV];
  __shared__ int s_act[MAX_KV];
  __shared__ int s_nact;
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  const long long row_g = (long long)rg * 128;                        // first output row of the work-group
  const long long row_l = row_g + wave * 32 + li;                     // the lane's output row
  const bool row_ok = row_l < p.M;
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * 4LL);
  const unsigned a_in = (unsigned)((MODE == 0 ? 4 : 8) * h * 4);      // byte offset of the lane's channels inside a 32-channel step
  const int ks = p.K >> 5;                                            // channel steps per offset

  // the offsets at which some row of the tile has a neighbour, in ascending order
  for (int k = tid; k < p.KV; k += 256) s_flag[k] = 0;
  __syncthreads();
  for (int k = 0; k < p.KV; ++k) {
    const int r = row_ok ? p.table[(long long)(p.rev ? p.KV - 1 - k : k) * p.M + row_l] : -1;
    if (__ballot(r >= 0) != 0ULL && l == 0) s_flag[k] = 1;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < p.KV; ++k)
      if (s_flag[k]) s_act[n++] = k;
    s_nact = n;
  }
  __syncthreads();
  const int S = s_nact * ks;                                          // contraction steps of this work-group

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

  // step s = (offset s / ks of the list, channels 32 (s % ks) ..): the lane's source row of a step, two steps ahead of its use
  auto row_of = [&](int s) -> int {
    if (s >= S || !row_ok) return -1;
    const int k = s_act[s / ks];
    return p.table[(long long)(p.rev ? p.KV - 1 - k : k) * p.M + row_l];
  };
  f32x4 an[4], bn[NB];
  auto load_a = [&](int s, int src) {
    const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 4u + a_in + (unsigned)((s % ks) * 128);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // mode 0: k = 8 g + 4 h + t; 16-bit: k = 16 (g / 2) + 8 h + 4 (g % 2) + t
      const int kofs = MODE == 0 ? 8 * g : 16 * (g >> 1) + 4 * (g & 1);
      an[g] = csn_bload4(ar, off + (unsigned)(kofs * 4));
    }
  };
  auto load_b = [&](int s) {
    const float* w = p.b + (long long)s_act[s / ks] * p.c_in * p.c_out;
    const int k0 = (s % ks) * 32;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = tid + 256 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if constexpr (!B_KN) {
        const int j = idx >> 3, kq = idx & 7;
        if (j0 + j < p.J) v = *reinterpret_cast<const f32x4*>(w + (long long)(j0 + j) * p.c_out + k0 + 4 * kq);
      } else {
        const int k = idx / (NB * 8), jq = idx % (NB * 8);
        if (j0 + 4 * jq < p.J) v = *reinterpret_cast<const f32x4*>(w + (long long)(k0 + k) * p.c_out + j0 + 4 * jq);
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

  int r1 = row_of(0);
  if (S > 0) { load_a(0, r1); load_b(0); }
  r1 = row_of(1);
  int r2 = row_of(2);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b();
    f32x4 af[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) { load_a(s + 1, r1); load_b(s + 1); }
    r1 = r2;
    r2 = row_of(s + 3);
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
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = j0 + nb * 32 + li;
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    const float bv = p.bias ? p.bias[col] : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = csn_acc_row(r, h);
      const float v = acc[nb][r] + bv;
      acc[nb][r] = v;
      if (rr < cnt) { p.c[(row_w + rr) * p.ldc + col] = v; sum += v; }
    }
    if (p.part) {
      // (mean, M2) of the wave's cnt rows, two passes over the registers (rows_gemm_kernel's epi == 1): the stored values are
      // untouched, the epilogue only adds
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
        const long long tile = (long long)rg * 4 + wave;
        p.part[(tile * 2) * p.J + col] = mu;
        p.part[(tile * 2 + 1) * p.J + col] = m2;
      }
    }
  }
}

// dW[k][ci][co] = sum_j x[fwd[k][j]][ci] dy[j][co] over the rows of one split-K chunk; see the file header.
// grid: x = 64-column blocks of c_out, y = 32 TA-row blocks of c_in, z = KV * splits (offset fastest)
template <int TA, int MODE>
__global__ __launch_bounds__(256) void sconv_wgrad_kernel(const float* __restrict__ x, int ldx, int n_in, const int* __restrict__ table,
                                                          const float* __restrict__ dy, int ldy, float* __restrict__ out, int n_out,
                                                          int c_in, int c_out, int KV, int chunk) {
  constexpr int TB = 2;
  __shared__ float red[TA * TB * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 32 * TA;
  const int kv = blockIdx.z % KV, split = blockIdx.z / KV;
  const int nbv = (c_out - co0) >= 64 ? 2 : 1;                        // column blocks of dy inside c_out (c_out % 32 == 0)
  const int quarter = chunk >> 2;                                     // chunk % 64 == 0
  const long long rb = (long long)split * chunk + (long long)wave * quarter;
  const long long left = (long long)n_out - rb;
  const csn_rsrc_t xr = csn_make_rsrc(x, ((long long)(n_in - 1) * ldx + c_in) * 4LL);
  const csn_rsrc_t yr = csn_make_rsrc(dy + rb * ldy, left > 0 ? ((left - 1) * ldy + c_out) * 4LL : 0LL);
  const int* tbl = table + (long long)kv * n_out + rb;
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
  int src[8];
  // the source rows of step st; returns whether any lane of the wave found one
  auto lookup = [&](int rr) -> bool {
    bool any = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + row_l + ROW_E * e;
      src[e] = row < left ? tbl[row] : -1;
      any |= src[e] >= 0;
    }
    return __ballot(any) != 0ULL;
  };
  auto load = [&](int rr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + row_l + ROW_E * e;
      const unsigned xo = src[e] < 0 ? CSN_OOB : ((unsigned)src[e] * (unsigned)ldx + (unsigned)(ci0 + li)) * 4u;
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) an[ta][e] = csn_bload(xr, xo + (unsigned)(ta * 128));
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) bn[tb][e] = tb < nbv ? csn_bload(yr, ((unsigned)row * (unsigned)ldy + (unsigned)(co0 + tb * 32 + li)) * 4u) : 0.f;
    }
  };
  const int n_steps = left <= 0 ? 0 : (int)((left < quarter ? left : quarter) + 15) / 16;
  bool any_n = false;
  if (n_steps > 0) {
    any_n = lookup(0);
    if (any_n) load(0);
  }
  for (int st = 0; st < n_steps; ++st) {
    const bool any_c = any_n;
    float af[TA][8], bf[TB][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) af[ta][e] = an[ta][e];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) bf[tb][e] = bn[tb][e];
    }
    any_n = false;
    if (st + 1 < n_steps) {
      any_n = lookup((st + 1) * 16);
      if (any_n) load((st + 1) * 16);
    }
    if (!any_c) continue;                                             // wave-uniform: no neighbour at this offset in these 16 rows
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
  float* o = out + ((long long)split * KV + kv) * c_in * c_out;
#pragma unroll
  for (int ta = 0; ta < TA; ++ta)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      if (tb >= nbv) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o[(long long)(ci0 + ta * 32 + csn_acc_row(r, h)) * c_out + co0 + tb * 32 + li] = acc[ta][tb][r];
    }
}

// fp64 column sums of 64-row chunks of dy: a lane owns a column, the four waves take every fourth row and are added in wave order
__global__ __launch_bounds__(256) void sconv_colsum_kernel(const float* __restrict__ dy, int ldy, long long n_rows, int C,
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
      for (long long r = r0 + w; r < r1; r += 4) s += (double)dy[r * ldy + c];
    sh[w][lane] = s;
    __syncthreads();
    if (w == 0 && ok) part[(long long)blockIdx.x * C + c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    __syncthreads();
  }
}

// the chunks' sums in chunk order: 32 columns x NSEG segments of the chunk list per work-group, segments added in order
constexpr int NSEG = 32;
__global__ __launch_bounds__(32 * NSEG) void sconv_colsum_merge_kernel(const double* __restrict__ part, int n_chunks, int C,
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

// ---- host side ---------------------------------------------------------------------------------------------------------
inline long long up256(long long b) { return (b + 255) & ~255LL; }
// rows of 32 c_in channels a work-group of the weight gradient owns: 4 where they divide c_in / 32, else the largest divisor
inline int wgrad_ta_for(int c_in) {
  const int t = c_in / 32;
  return t % 4 == 0 ? 4 : (t % 3 == 0 ? 3 : (t % 2 == 0 ? 2 : 1));
}

// split-K of the weight gradient: about one work-group per CU over (offset, tile, chunk); chunks of a multiple of 64 rows
void wgrad_split(long long n_rows, int kv, int c_in, int c_out, int& splits, int& chunk) {
  const long long tiles = (long long)kv * ((c_out + 63) / 64) * (c_in / (32 * wgrad_ta_for(c_in)));
  const long long want = (TARGET_GROUPS + tiles - 1) / tiles;
  long long ch = ((n_rows + want - 1) / want + 63) / 64 * 64;
  if (ch > 65536) ch = 65536;
  chunk = (int)ch;
  splits = (int)((n_rows + ch - 1) / ch);
}

struct WsLayout { long long part, slabs, total; };

WsLayout ws_layout(long long n_out, int kv, int c_in, int c_out) {
  WsLayout L{};
  long long o = 0;
  L.part = o;  o += up256(((n_out + 63) / 64) * c_out * (long long)sizeof(double));
  int splits, chunk;
  wgrad_split(n_out, kv, c_in, c_out, splits, chunk);
  L.slabs = o; if (splits > 1) o += up256((long long)splits * kv * c_in * c_out * (long long)sizeof(float));
  L.total = o;
  return L;
}

template <int NB, bool B_KN>
int launch_gemm_nb(const SconvGemmP& p, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * ((p.M + 127) / 128);
  if (groups > 0x7fffffffLL) return -5;
  const dim3 grid((unsigned)groups), block(256);
  if (mode == 0) hipLaunchKernelGGL((sconv_gemm_kernel<NB, 0, B_KN>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((sconv_gemm_kernel<NB, 1, B_KN>), grid, block, 0, st, p);
  return (int)hipGetLastError();
}

// the wave owns every column up to 128; wider outputs take two column groups of the smallest width that covers them.  Where
// that leaves fewer than TARGET_GROUPS work-groups (the coarse levels: few rows, wide rows), the column groups are halved
// until it does not: more work-groups gather the same rows (from L2), each contracts a narrower slice.  The sums are the same.
// csn_dev_set(CSN_DEV_SCONV_NB, 1..4) pins the column blocks per wave instead (tests reach every instance at small sizes).
template <bool B_KN>
int launch_gemm(const SconvGemmP& p, int mode, hipStream_t st) {
  const int t = p.J / 32;
  int nb = t <= 4 ? t : (t + 1) / 2;
  const long long row_groups = ((long long)p.M + 127) / 128;
  while (nb > 1 && row_groups * ((t + nb - 1) / nb) < TARGET_GROUPS) nb = (nb + 1) / 2;
  if (csn_dev_sconv_nb > 0) nb = csn_dev_sconv_nb < t ? csn_dev_sconv_nb : t;
  switch (nb) {
    case 1: return launch_gemm_nb<1, B_KN>(p, mode, st);
    case 2: return launch_gemm_nb<2, B_KN>(p, mode, st);
    case 3: return launch_gemm_nb<3, B_KN>(p, mode, st);
    default: return launch_gemm_nb<4, B_KN>(p, mode, st);
  }
}

template <int TA>
int launch_wgrad_ta(const CsnSparseConvArgs& a, float* out, int splits, int chunk, int mode, hipStream_t st) {
  const dim3 grid((unsigned)((a.c_out + 63) / 64), (unsigned)(a.c_in / (32 * TA)), (unsigned)(splits * a.kv)), block(256);
  if (mode == 0)
    hipLaunchKernelGGL((sconv_wgrad_kernel<TA, 0>), grid, block, 0, st, a.x, a.ld_x, a.n_in, a.fwd_table, a.dy, a.ld_dy, out, a.n_out,
                       a.c_in, a.c_out, a.kv, chunk);
  else
    hipLaunchKernelGGL((sconv_wgrad_kernel<TA, 1>), grid, block, 0, st, a.x, a.ld_x, a.n_in, a.fwd_table, a.dy, a.ld_dy, out, a.n_out,
                       a.c_in, a.c_out, a.kv, chunk);
  return (int)hipGetLastError();
}

}  // namespace

int csn_dev_sconv_nb = 0;

long long csn_sparse_conv_ws_bytes(long long n_in, long long n_out, int kv, int c_in, int c_out, int backward) {
  (void)n_in;
  return backward ? ws_layout(n_out, kv, c_in, c_out).total : 0;
}

int csn_launch_sparse_conv_fwd(const CsnSparseConvArgs& a, int mode, hipStream_t st) {
  mode = mode != 0;
  SconvGemmP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv; p.bias = a.bias;
  return launch_gemm<true>(p, mode, st);
}

long long csn_sparse_conv_stats_ws_bytes(long long n_out, int c_out) {
  return up256(((n_out + 127) / 128) * 4 * 2 * c_out * (long long)sizeof(float));
}

// the forward product with the statistics epilogue, then the tiles' (mean, M2) merged in fp64 in a fixed order (rows_bn_act.hip)
int csn_launch_sparse_conv_stats_fwd(const CsnSparseConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                     float eps, float momentum, int mode, hipStream_t st) {
  mode = mode != 0;
  SconvGemmP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv; p.bias = nullptr;
  p.part = static_cast<float*>(a.ws);
  if (const int e = launch_gemm<true>(p, mode, st)) return e;
  const int n_tiles = (int)(((long long)a.n_out + 127) / 128) * 4;
  return csn_launch_bn_stats_merge(p.part, n_tiles, a.n_out, a.c_out, eps, momentum, mean, invstd, running_mean, running_var, st);
}

int csn_launch_sparse_conv_bwd(const CsnSparseConvArgs& a, int mode, hipStream_t st) {
  mode = mode != 0;
  const WsLayout L = ws_layout(a.n_out, a.kv, a.c_in, a.c_out);
  char* ws = static_cast<char*>(a.ws);
  if (a.dx) {
    // dx[i] = sum_k dy[bwd[k][i]] W[k]^T: the forward kernel over the input rows, contraction over c_out
    SconvGemmP p{};
    // bwd_table NULL (n_in == n_out, checked by the caller): the stride-1 identity bwd[k] = fwd[KV - 1 - k] on the forward table
    p.a = a.dy; p.lda = a.ld_dy; p.n_src = a.n_out; p.table = a.bwd_table ? a.bwd_table : a.fwd_table; p.rev = a.bwd_table == nullptr;
    p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
    p.c = a.dx; p.ldc = a.ld_dx; p.M = a.n_in; p.K = a.c_out; p.J = a.c_in; p.KV = a.kv; p.bias = nullptr;
    if (const int e = launch_gemm<false>(p, mode, st)) return e;
  }
  if (a.dbias) {
    double* part = reinterpret_cast<double*>(ws + L.part);
    const int n_chunks = (int)(((long long)a.n_out + 63) / 64);
    hipLaunchKernelGGL(sconv_colsum_kernel, dim3(n_chunks), dim3(256), 0, st, a.dy, a.ld_dy, (long long)a.n_out, a.c_out, part);
    if (const int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(sconv_colsum_merge_kernel, dim3(a.c_out / 32), dim3(32 * NSEG), 0, st, part, n_chunks, a.c_out, a.dbias);
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (a.dw) {
    int splits, chunk;
    wgrad_split(a.n_out, a.kv, a.c_in, a.c_out, splits, chunk);
    float* out = splits > 1 ? reinterpret_cast<float*>(ws + L.slabs) : a.dw;
    int e;
    switch (wgrad_ta_for(a.c_in)) {
      case 1: e = launch_wgrad_ta<1>(a, out, splits, chunk, mode, st); break;
      case 2: e = launch_wgrad_ta<2>(a, out, splits, chunk, mode, st); break;
      case 3: e = launch_wgrad_ta<3>(a, out, splits, chunk, mode, st); break;
      default: e = launch_wgrad_ta<4>(a, out, splits, chunk, mode, st); break;
    }
    if (e) return e;
    if (splits > 1) return csn_launch_slab_reduce(out, a.dw, splits, (long long)a.kv * a.c_in * a.c_out, 1.f, 0, st);
  }
  return 0;
}
