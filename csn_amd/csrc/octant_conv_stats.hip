// The octant products of octant_conv.hip with a BatchNorm statistics epilogue (include/csn_hip.h section 26): the training forward
// of the Res16UNets' eight resolution changes, z = the product without a bias and, from the accumulators of the same launch, the
// (mean, M2) of every wave's rows — merged in fp64 in a fixed order into mean, invstd and the running statistics, as (15a) does
// for the gather-GEMM.
//
//   down               the gather form over children[8][n_coarse]: sparse_conv.hip's statistics launcher as it is (a table of 8
//                      offsets; store_tile's epilogue, bn_stats_merge).  No kernel of its own.
//   octant_rows_stats_kernel<NB, MODE>   up: octant_rows_body.inc with its third epilogue.  A work-group's tile of <= 128 entries of
//                      `order` lies inside ONE octant segment, so a wave's tile holds 0 .. 32 rows wherever it sits in the grid and
//                      its rows leave for permuted destinations (s_dst).  The wave forms (mean, M2) over the rows whose destination
//                      exists — two passes over the registers, as store_tile — and stores its own row count beside them:
//                      part[tile][2][J], cnt[tile], tile = 4 * row group + wave.  A row group without a span writes four zero
//                      counts and leaves, so every count of the grid is written by every launch and none is assumed.
//   octant_stats_merge_kernel   chan_walk_counts (rows_mma.h): the tiles merged by Chan's formula with each tile's stored count, 64
//                      segments of the tile list per column, the segments in bn_stats_merge's pairwise tree; bn_finish.
// z holds the bits of csn_launch_octant_up_fwd / _down_fwd with bias = NULL: the loop is the same text and the stored value is
// acc + 0.f either way.  No floating-point atomics: two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

struct OctRowsStatsP {
  const float* a; int lda; int n_src;   // A[n_src][lda]: the gathered (coarse) map
  const int* parent;                    // [M]
  const int* order;                     // [M] rows sorted by (octant, row)
  const int* seg;                       // [9]
  const float* b;                       // W[8][c_in][c_out]
  int c_in, c_out;
  float* c; int ldc;                    // C[M][ldc]
  int M, K, J;
  const float* bias;                    // NULL: a convolution in front of a BatchNorm has none
  float* part;                          // [tile][2][J]: (mean, M2) of each wave's rows
  int* cnt;                             // [tile]: the rows they are taken over
};

// named by the body's inference epilogue, which no instance here takes: declared, never defined or called
__device__ const OctRowsStatsP* oct_bn_args_late();

// grid: column groups of NB * 32 fastest, then ceil(M / 128) + 7 row groups
template <int NB, int MODE>
__global__ __launch_bounds__(256) void octant_rows_stats_kernel(const OctRowsStatsP p) {
  constexpr bool B_KN = true, BN = NB < 0, STATS = NB > 0;
#include "octant_rows_body.inc"
}

constexpr int SCOLS = 16, SSEG = 64;    // rows_bn_act.hip's merge shape: 16 columns x 64 segments of the tile list per work-group

__global__ __launch_bounds__(SCOLS * SSEG) void octant_stats_merge_kernel(const float* __restrict__ part, const int* __restrict__ cnt,
                                                                          int n_tiles, int C, float eps, float momentum,
                                                                          float* __restrict__ mean, float* __restrict__ invstd,
                                                                          float* __restrict__ rmean, float* __restrict__ rvar) {
  __shared__ double sh[3][SSEG][SCOLS];
  const int lc = threadIdx.x % SCOLS, sg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  const int per = (n_tiles + SSEG - 1) / SSEG;
  const int t0 = min(n_tiles, sg * per), t1 = min(n_tiles, t0 + per);
  double n = 0.0, mu = 0.0, m2 = 0.0;
  chan_walk_counts(n, mu, m2, part, cnt, t0, t1, C, col);
  for (int stride = 1; stride < SSEG; stride <<= 1) {
    sh[0][sg][lc] = n; sh[1][sg][lc] = mu; sh[2][sg][lc] = m2;
    __syncthreads();
    if (sg % (2 * stride) == 0) chan_merge(n, mu, m2, sh[0][sg + stride][lc], sh[1][sg + stride][lc], sh[2][sg + stride][lc]);
    __syncthreads();
  }
  if (sg == 0) bn_finish(n, mu, m2, col, eps, momentum, mean, invstd, rmean, rvar);
}

inline long long up_tiles(long long n_fine) { return ((n_fine + 127) / 128 + 7) * 4; }

struct WsLayout { long long part, cnt, total; };

WsLayout up_layout(long long n_fine, int c_out) {
  WsLayout L{};
  long long o = 0;
  L.part = o; o += up256(up_tiles(n_fine) * 2 * c_out * (long long)sizeof(float));
  L.cnt = o;  o += up256(up_tiles(n_fine) * (long long)sizeof(int));
  L.total = o;
  return L;
}

template <int NB>
int launch_up_nb(const OctRowsStatsP& p, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128 + 7);
  if (groups > 0x7fffffffLL) return -5;
  auto* const k = mode == 0 ? octant_rows_stats_kernel<NB, 0> : octant_rows_stats_kernel<NB, 1>;
  hipLaunchKernelGGL(k, dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace

long long csn_octant_stats_ws_bytes(long long n_fine, long long n_coarse, int c_out, int up) {
  return up ? up_layout(n_fine, c_out).total : csn_sparse_conv_stats_ws_bytes(n_coarse, c_out);
}

// mode: 0 fp32, anything else bf16x3, as csn_launch_octant_down_fwd
int csn_launch_octant_down_stats_fwd(const CsnOctantConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                     float eps, float momentum, int mode, hipStream_t st) {
  CsnSparseConvArgs g{};
  g.kv = 8; g.c_in = a.c_in; g.c_out = a.c_out; g.w = a.w;
  g.x = a.x; g.ld_x = a.ld_x; g.n_in = a.n_fine; g.fwd_table = a.children; g.n_out = a.n_coarse; g.y = a.y; g.ld_y = a.ld_y; g.ws = a.ws;
  return csn_launch_sparse_conv_stats_fwd(g, nullptr, 0, mean, invstd, running_mean, running_var, eps, momentum, mode != 0, st);
}

int csn_launch_octant_up_stats_fwd(const CsnOctantConvArgs& a, float* mean, float* invstd, float* running_mean, float* running_var,
                                   float eps, float momentum, int mode, hipStream_t st) {
  const WsLayout L = up_layout(a.n_fine, a.c_out);
  char* ws = static_cast<char*>(a.ws);
  OctRowsStatsP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_coarse; p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.b = a.w;
  p.c_in = a.c_in; p.c_out = a.c_out; p.c = a.y; p.ldc = a.ld_y; p.M = a.n_fine; p.K = a.c_in; p.J = a.c_out; p.bias = nullptr;
  p.part = reinterpret_cast<float*>(ws + L.part); p.cnt = reinterpret_cast<int*>(ws + L.cnt);
  if (const int e = dispatch4(csn_octant_column_blocks(p.J, p.M), [&](auto nb) { return launch_up_nb<nb()>(p, mode != 0, st); })) return e;
  hipLaunchKernelGGL(octant_stats_merge_kernel, dim3(a.c_out / SCOLS), dim3(SCOLS * SSEG), 0, st, p.part, p.cnt, (int)up_tiles(a.n_fine),
                     a.c_out, eps, momentum, mean, invstd, running_mean, running_var);
  return (int)hipGetLastError();
}
