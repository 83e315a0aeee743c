// The HRNet backbone's training step on bf16 activation maps (include/csn_hip.h section 28, tuning.train_maps16): the four launches
// of a fused layer — sections 15a, 15b forward, 15b backward and the weight gradient of section 14 — with the ReLU output y between
// them stored as bf16 rows.  In math mode 2 with csn_set_thread_rows16 the convolution and its weight gradient round y to bf16
// before their products anyway, so a map that already holds those bits changes no product; z, the statistics and every gradient
// map stay fp32.
//
//   sconv_stats_x16_kernel<NB>      (15a) on a bf16 x: the loop of sconv_a16_body.inc (sparse_conv_maps16.hip's, A fragments loaded as
//                      they lie: two 16-byte loads per step) with store_tile's statistics epilogue — z and the (mean, M2) partials are
//                      the bits of sconv_gemm16_kernel<NB, false, true> fed the same values as fp32; then rows_bn_act.hip's merge.
//   rows_bn_act_fwd16_kernel<R16, Y16>   (15b)'s row walk; v is formed as there (r first, the terms in order, the ReLU) and stored as
//                      to16(v), one rounding to nearest even, in 8-byte stores; a bf16 r is read in 8-byte loads and widened exactly.
//   rows_bn_act_bwd16_kernel<PASS>  (15b)'s two passes (bwd_span of rows_bn_act_body.inc) with the mask g' = dy [y16 > 0] read from
//                      8-byte runs of y; the chunk sums, their order and the sums launch are rows_bn_act.hip's.
//   sconv_wgrad_x16_kernel<TA>      sconv_wgrad16_kernel's steps on a bf16 x.  A lane's A fragment is ONE channel of 8 gathered rows: read
//                      straight from 16-bit rows that would be eight 2-byte loads.  Instead the wave loads the step's 16 rows x 32 TA
//                      channels in 16-byte pieces (a lane per piece: 4 TA pieces a row, TA loads a lane), stages them in a tile of
//                      its own in LDS and reads the fragments back transposed (ds_read_b64_tr_b16, two per fragment: rows 8 h .. 8 h +
//                      3 and 8 h + 4 .. 8 h + 7 of column li).  The tile's pitch is 16, 48 or 80 dwords (16 mod 32), so that the four rows of a
//                      transposed read fall on distinct banks.  The rows of a step, the skip ballot (a step none of whose 16 rows has
//                      a neighbour), the split-K chunks, the wave reduction and the slab reduction are sconv_wgrad16_kernel's: dW is the
//                      bits of csn_sparse_conv_bwd_f32 in mode 2 fed the same values.  The tiles lie in the reduction's LDS buffer,
//                      which is not used before the loop ends.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

constexpr int MAX_KV = 125;
typedef s16x4 __attribute__((address_space(3))) * lds_s16x4p;

// ---- (28a) convolution + statistics on a bf16 x ------------------------------------------------------------------------
struct SconvStatsX16P {
  const void* a; int lda; int n_src;   // A[n_src][lda]: the gathered map, bf16 rows, pitch in elements
  const int* table;                    // [KV][M]
  const float* b;                      // W[KV][c_in][c_out]
  int c_in, c_out;
  float* c; int ldc;                   // z[M][J], fp32
  int M, K, J, KV;
  float* part;                         // the (mean, M2) of each wave's rows, [tile][2][J], tile = 32 rows
};

template <int NB>
__global__ __launch_bounds__(256) void sconv_stats_x16_kernel(const SconvStatsX16P p) {
  constexpr bool H16 = false, A16 = true;
  constexpr int MODE = 2;
#include "sconv_a16_body.inc"

  const long long row_w = row_g + wave * 32;                          // first row of the wave's tile
  const int cnt = (int)(p.M - row_w < 32 ? (p.M - row_w < 0 ? 0 : p.M - row_w) : 32);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = j0 + nb * 32 + li;
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    store_tile(acc[nb], 0.f, p.c, p.ldc, row_w, cnt, col, h, true, p.part, (long long)rg * 4 + wave, p.J);
  }
}

template <int NB>
int launch_stats_nb(const SconvStatsX16P& p, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128);
  if (groups > 0x7fffffffLL) return -5;
  hipLaunchKernelGGL(sconv_stats_x16_kernel<NB>, dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// ---- (28b, 28c) BatchNorm apply + sum + residual + ReLU with y / r as bf16 rows -------------------------------------------
#include "rows_bn_act_body.inc"

// rows_bn_act_fwd_kernel with r read as (R16) and y written as (Y16) bf16 rows
template <bool R16, bool Y16>
__global__ __launch_bounds__(256) void rows_bn_act_fwd16_kernel(const BnActP p) {
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
      is[m][e] = in ? inv_std(p, m, t.c + e, p.eval) : 0.f;
      ga[m][e] = in ? p.gamma[m][t.c + e] : 0.f;
      be[m][e] = in ? p.beta[m][t.c + e] : 0.f;
    }
#pragma unroll 2
  for (int rr = t.rl; rr < rows; rr += t.RL) {
    const long long row = r0 + rr;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (p.r) {
      if constexpr (R16) o = from16x4<false>(*reinterpret_cast<const s16x4*>(reinterpret_cast<const short*>(p.r) + row * p.ld_r + t.c));
      else o = *reinterpret_cast<const f32x4*>(p.r + row * p.ld_r + t.c);
    }
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
    if constexpr (Y16) *reinterpret_cast<s16x4*>(reinterpret_cast<short*>(p.y) + row * p.ld_y + t.c) = to16x4<false>(o);
    else *reinterpret_cast<f32x4*>(p.y + row * p.ld_y + t.c) = o;
  }
}

// rows_bn_act_bwd_kernel<PASS, false> with the mask read from bf16 rows
template <int PASS>
__global__ __launch_bounds__(256) void rows_bn_act_bwd16_kernel(const BnActP p) {
  __shared__ double sh[PASS == 1 ? (1 + MAXT) * 1024 : 1];                  // [q][row lane][C]: row lanes * C <= 1024
  const Lane t = lane_of(p.C);
  const long long r0 = (long long)blockIdx.x * 64;
  const int rows = (int)(p.n_rows - r0 < 64 ? p.n_rows - r0 : 64);
  bwd_span<PASS, true>(p, t, r0, t.rl, rows, 0, p.eval, sh);
  if constexpr (PASS == 1) store_part(p, t, blockIdx.x, sh);
}

int bwd_pass_y16(int pass, const CsnRowsBnActArgs& a, const int*, int, double* part, const float* coef, int n_parts, hipStream_t st) {
  BnActP p = make_p(a, nullptr, 0);
  p.part = part; p.coef = coef; p.n_parts = n_parts;
  const int n_chunks = (int)(((long long)a.n_rows + 63) / 64);
  hipLaunchKernelGGL((pass == 1 ? rows_bn_act_bwd16_kernel<1> : rows_bn_act_bwd16_kernel<2>), dim3(n_chunks), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// ---- (28d) weight gradient on a bf16 gathered x --------------------------------------------------------------------------
// shorts per row of a wave's staged tile (16 rows x 32 TA channels): 16, 48, 80 dwords — 16 mod 32, so the four 16-dword rows of a
// transposed read start at 0, 16, 32 and 48 mod 64 in some order
template <int TA> constexpr int x_pitch = TA == 1 ? 32 : (TA == 2 ? 96 : 160);

// grid: x = 64-column blocks of c_out, y = 32 TA-row blocks of c_in, z = KV * splits (offset fastest), as sconv_wgrad16_kernel
template <int TA>
__global__ __launch_bounds__(256) void sconv_wgrad_x16_kernel(const short* __restrict__ x, int ldx, int n_in, const int* __restrict__ table,
                                                              const float* __restrict__ dy, int ldy, float* __restrict__ out, int n_out,
                                                              int c_in, int c_out, int KV, int chunk) {
  constexpr int XP = x_pitch<TA>, PR = 4 * TA;                        // PR: 16-byte pieces per staged row
  static_assert(4 * 16 * XP * 2 <= TA * WG_TB * 16 * 64 * 4, "the four waves' tiles lie inside red");
  __shared__ __attribute__((aligned(16))) float red[TA * WG_TB * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 32 * TA;
  const int kv = blockIdx.z % KV, split = blockIdx.z / KV;
  const int nbv = (c_out - co0) >= 64 ? 2 : 1;                        // column blocks of dy inside c_out (c_out % 32 == 0)
  const int quarter = chunk >> 2;                                     // chunk % 64 == 0
  const long long rb = (long long)split * chunk + (long long)wave * quarter;
  const long long left = (long long)n_out - rb;
  const csn_rsrc_t xr = csn_make_rsrc(x, ((long long)(n_in - 1) * ldx + c_in) * 2LL);
  const csn_rsrc_t yr = csn_make_rsrc(dy + rb * ldy, left > 0 ? ((left - 1) * ldy + c_out) * 4LL : 0LL);
  const int* tbl = table + (long long)kv * n_out + rb;
  short* xs = reinterpret_cast<short*>(red) + wave * 16 * XP;          // the wave's tile
  // the lane's address of a transposed read: row 8 h + q, columns 16 (li / 16) + 4 p .. + 3 for lane 4 q + p of its 16-lane group
  const short* xt = xs + (8 * h + ((l >> 2) & 3)) * XP + 16 * ((l >> 4) & 1) + 4 * (l & 3);

  f32x16 acc[TA][WG_TB] = {};
  f32x4 xn[TA];
  float bn[WG_TB][8];
  int src[TA];
  // the source rows of the lane's pieces of the step at row rr; returns whether any lane of the wave found one (the pieces cover
  // the step's 16 rows: sconv_wgrad_body's predicate)
  auto lookup = [&](int rr) -> bool {
    bool any = false;
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      const int row = rr + (l + 64 * i) / PR;
      src[i] = row < left ? tbl[row] : -1;
      any |= src[i] >= 0;
    }
    return __ballot(any) != 0ULL;
  };
  auto load = [&](int rr) {
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      const int pc = (l + 64 * i) % PR;
      xn[i] = csn_bload4(xr, src[i] < 0 ? CSN_OOB : ((unsigned)src[i] * (unsigned)ldx + (unsigned)(ci0 + 8 * pc)) * 2u);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + wgrad_row<2>(h, e);
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bn[tb][e] = tb < nbv ? csn_bload(yr, ((unsigned)row * (unsigned)ldy + (unsigned)(co0 + tb * 32 + li)) * 4u) : 0.f;
    }
  };
  const int n_steps = wgrad_steps(left, quarter);
  bool any_n = false;
  if (n_steps > 0) {
    any_n = lookup(0);
    if (any_n) load(0);
  }
  for (int st = 0; st < n_steps; ++st) {
    const bool any_c = any_n;
    f32x4 xf[TA];
    float bf[WG_TB][8];
#pragma unroll
    for (int i = 0; i < TA; ++i) xf[i] = xn[i];
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bf[tb][e] = bn[tb][e];
    any_n = false;
    if (st + 1 < n_steps) {
      any_n = lookup((st + 1) * 16);
      if (any_n) load((st + 1) * 16);
    }
    if (!any_c) continue;                                             // wave-uniform: no neighbour at this offset in these 16 rows
    // through the wave's tile: pieces in, fragments out.  One wave's LDS accesses are served in order; the fences keep the
    // compiler from moving them across each other
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      const int idx = l + 64 * i;
      *reinterpret_cast<f32x4*>(xs + (idx / PR) * XP + 8 * (idx % PR)) = xf[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    s16x8 a16[TA];
#pragma unroll
    for (int ta = 0; ta < TA; ++ta)
      a16[ta] = join8(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(xt + 32 * ta)),
                      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(xt + 32 * ta + 4 * XP)));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    wgrad_step_a16<TA>(acc, a16, bf, nbv);
  }
  __syncthreads();                                                    // every wave is done with its tile: red is the reduction's
  wgrad_reduce_store<TA>(acc, red, out + ((long long)split * KV + kv) * c_in * c_out, c_out, ci0, co0, nbv, wave, l);
}

template <int TA>
int launch_wgrad_ta(const CsnSparseConvArgs& a, float* out, int splits, int chunk, hipStream_t st) {
  const dim3 grid((unsigned)((a.c_out + 63) / 64), (unsigned)(a.c_in / (32 * TA)), (unsigned)(splits * a.kv)), block(256);
  hipLaunchKernelGGL(sconv_wgrad_x16_kernel<TA>, grid, block, 0, st, reinterpret_cast<const short*>(a.x), a.ld_x, a.n_in, a.fwd_table, a.dy,
                     a.ld_dy, out, a.n_out, a.c_in, a.c_out, a.kv, chunk);
  return (int)hipGetLastError();
}

}  // namespace

int csn_launch_sparse_conv_stats_fwd_x16(const CsnSparseConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                         float eps, float momentum, hipStream_t st) {
  SconvStatsX16P p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv;
  p.part = static_cast<float*>(a.ws);
  if (const int e = dispatch4(csn_sconv_column_blocks(p.J, p.M), [&](auto nb) { return launch_stats_nb<nb()>(p, st); })) return e;
  const int n_tiles = (int)(((long long)a.n_out + 127) / 128) * 4;
  return csn_launch_bn_stats_merge(p.part, n_tiles, a.n_out, a.c_out, eps, momentum, a.y, a.ld_y, nullptr, 0, mean, invstd, running_mean,
                                   running_var, st);
}

int csn_launch_sparse_conv_wgrad_x16(const CsnSparseConvArgs& a, hipStream_t st) {
  int ta, splits, chunk;
  long long slabs;
  csn_sconv_wgrad_plan(a.n_out, a.kv, a.c_in, a.c_out, &ta, &splits, &chunk, &slabs);
  float* out = splits > 1 ? reinterpret_cast<float*>(static_cast<char*>(a.ws) + slabs) : a.dw;
  if (const int e = dispatch4(ta, [&](auto t) { return launch_wgrad_ta<t()>(a, out, splits, chunk, st); })) return e;
  if (splits > 1) return csn_launch_slab_reduce(out, a.dw, splits, (long long)a.kv * a.c_in * a.c_out, 1.f, 0, st);
  return 0;
}

int csn_launch_rows_bn_act_fwd16(const CsnRowsBnActArgs& a, int r16, int y16, hipStream_t st) {
  if (!y16 && !(a.r && r16)) return csn_launch_rows_bn_act_fwd(a, nullptr, 0, st);        // nothing 16-bit: (15b) itself
  const BnActP p = make_p(a, nullptr, 0);
  const unsigned n_chunks = (unsigned)(((long long)a.n_rows + 63) / 64);
  void (*const k[2][2])(BnActP) = {{nullptr, rows_bn_act_fwd16_kernel<false, true>},
                                   {rows_bn_act_fwd16_kernel<true, false>, rows_bn_act_fwd16_kernel<true, true>}};
  hipLaunchKernelGGL(k[a.r && r16][y16 != 0], dim3(n_chunks), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

int csn_launch_rows_bn_act_bwd16(const CsnRowsBnActArgs& a, hipStream_t st) {
  return csn_launch_rows_bn_act_bwd(a, nullptr, 0, st, bwd_pass_y16);
}
