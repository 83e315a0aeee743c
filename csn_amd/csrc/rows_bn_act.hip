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
//
// The backward's passes, its sums and the tile merge are stated ONCE, each as a __device__ body over a span of rows (of parts, of
// tiles) and an offset into the statistics, for the two forms of the BatchNorm batch.  (15) the whole map: the body once, on the
// work-group's whole chunk (the whole part / tile list) at offset 0; no group offsets are read, and the eval path (running
// statistics and eps) is kept.  (20, training only) per contiguous ROW GROUP: group g is the rows [group_rows[g], group_rows[g + 1])
// and has its own (mu, s) at offset g * C.  A work-group walks the groups that meet its 64 rows one after the other and calls the
// body per span, which loads that group's per-column constants; the backward's chunk sums are cut at the group boundaries (at most
// chunks + G - 1 parts), added per group and the groups in ascending order; the merge takes the whole 32-row tiles of a group
// from the epilogue's partials and re-reads the <= 31 rows of a tile that a boundary cuts from z.  rows_bn_act_bwd and
// rows_bn_act_sums are templates on GROUPED; bn_stats_merge / bn_stats_merge_groups are two kernels on the one merge_tiles, and
// the forward has two kernels of its own, rows_bn_act_fwd / rows_bn_act_groups_fwd (see there for why).  With one group every sum
// is the whole-map sum in the same order: the same bits.  A row outside every group is not touched, and no row or part index
// leaves its array whatever group_rows holds.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

#include "rows_bn_act_body.inc"

// the rows [lo, hi) of the work-group's chunk (rows from r0) that belong to group g; false: none
__device__ __forceinline__ bool group_span(const BnActP& p, int g, long long r0, int rows, int& lo, int& hi) {
  const long long a = (long long)p.grp[g], b = (long long)p.grp[g + 1];
  lo = (int)(a > r0 ? (a < r0 + rows ? a - r0 : rows) : 0);
  hi = (int)(b < r0 + rows ? (b > r0 ? b - r0 : 0) : rows);
  return lo < hi;
}
// a row lane's first row at or after lo
__device__ __forceinline__ int first_row(const Lane& t, int lo) { return t.rl >= lo ? t.rl : t.rl + (lo - t.rl + t.RL - 1) / t.RL * t.RL; }

// number of the part that chunk `chunk` and group g share: one more per chunk and per group, less the boundaries that fall on a
// chunk edge (there the chunk and the group change together)
__device__ __forceinline__ int part_index(const int* grp, int g, long long chunk) {
  int on_edge = 0;
  for (int j = 1; j <= g; ++j) on_edge += (grp[j] & 63) == 0;
  return (int)chunk + g - on_edge;
}

// The forward keeps a kernel of its own for the whole map and for row groups: on one shared row loop the whole-map kernel measured
// slower than as written here (profiles/rows_bn_act_ab_time.txt), and with the group's constants loaded the way the whole-map
// kernel loads them the row-group kernel loses a wave per SIMD.
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
      is[m][e] = in ? inv_std(p, m, t.c + e, p.eval) : 0.f;
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

// the same per group span of the chunk: gamma / beta once, a group's (mu, s) when the work-group enters it
__global__ __launch_bounds__(256) void rows_bn_act_groups_fwd_kernel(const BnActP p) {
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
      ga[m][e] = in ? p.gamma[m][t.c + e] : 0.f;
      be[m][e] = in ? p.beta[m][t.c + e] : 0.f;
    }
  for (int g = 0; g < p.G; ++g) {
    int lo, hi;
    if (!group_span(p, g, r0, rows, lo, hi)) continue;
#pragma unroll
    for (int m = 0; m < MAXT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = m < p.M;
        mu[m][e] = in ? p.mean[m][g * p.C + t.c + e] : 0.f;
        is[m][e] = in ? p.scale[m][g * p.C + t.c + e] : 0.f;
      }
#pragma unroll 2
    for (int rr = first_row(t, lo); rr < hi; rr += t.RL) {
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
}


template <int PASS, bool GROUPED>
__global__ __launch_bounds__(256) void rows_bn_act_bwd_kernel(const BnActP p) {
  __shared__ double sh[PASS == 1 ? (1 + MAXT) * 1024 : 1];                  // [q][row lane][C]: row lanes * C <= 1024
  const Lane t = lane_of(p.C);
  const long long r0 = (long long)blockIdx.x * 64;
  const int rows = (int)(p.n_rows - r0 < 64 ? p.n_rows - r0 : 64);
  if constexpr (!GROUPED) {
    bwd_span<PASS>(p, t, r0, t.rl, rows, 0, p.eval, sh);
    if constexpr (PASS == 1) store_part(p, t, blockIdx.x, sh);
  } else {
    for (int g = 0; g < p.G; ++g) {
      int lo, hi;
      if (!group_span(p, g, r0, rows, lo, hi)) continue;                    // uniform over the work-group
      bwd_span<PASS>(p, t, r0, first_row(t, lo), hi, g * p.C, false, sh);
      if constexpr (PASS == 1) {
        // the part index AFTER the row loop: formed before it, the offsets' scalar loads hold back the first row loads
        const int pi = part_index(p.grp, g, blockIdx.x);
        if (pi >= 0 && pi < p.n_parts) store_part(p, t, pi, sh);
        __syncthreads();                                                    // sh is the next group's
      }
    }
  }
}

constexpr int SCOLS = 16, SSEG = 64;

// (n, mean, M2) of the tiles [ta, tb) of a convolution's statistics epilogue, for 16 columns x 64 segments of that tile list per
// work-group: a thread merges its segment's tiles in tile order, the segments are merged pairwise in a fixed tree (neighbours
// first, the lower tiles on the left).  The result is segment 0's.
__device__ __forceinline__ void merge_tiles(double& n, double& mu, double& m2, const float* __restrict__ part, int ta, int tb, int n_rows,
                                            int C, int col, int seg, int lc, double (*sh)[SSEG][SCOLS]) {
  const int per = (tb - ta + SSEG - 1) / SSEG;
  const int t0 = ta + seg * per, t1 = min(tb, t0 + per);
  chan_walk(n, mu, m2, part, t0, t1, n_rows, C, col);
  for (int stride = 1; stride < SSEG; stride <<= 1) {
    sh[0][seg][lc] = n; sh[1][seg][lc] = mu; sh[2][seg][lc] = m2;
    __syncthreads();
    if (seg % (2 * stride) == 0) chan_merge(n, mu, m2, sh[0][seg + stride][lc], sh[1][seg + stride][lc], sh[2][seg + stride][lc]);
    __syncthreads();
  }
}

// The tiles' (mean, M2) -> mean, invstd, running statistics of the whole map.  (Two kernels on the one merge_tiles: the whole-map
// kernel keeps the arguments it had; as an instance that also takes z and the offsets it measured 0.4 % slower.)
__global__ __launch_bounds__(SCOLS * SSEG) void bn_stats_merge_kernel(const float* __restrict__ part, int n_tiles, int n_rows, int C,
                                                                       float eps, float momentum, float* __restrict__ mean,
                                                                       float* __restrict__ invstd, float* __restrict__ rmean,
                                                                       float* __restrict__ rvar) {
  __shared__ double sh[3][SSEG][SCOLS];
  const int lc = threadIdx.x % SCOLS, seg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  merge_tiles(n, mu, m2, part, 0, n_tiles, n_rows, C, col, seg, lc, sh);
  if (seg == 0) bn_finish(n, mu, m2, col, eps, momentum, mean, invstd, rmean, rvar);
}

// The same per group, the groups one after the other (the running statistics take G updates in group order).  A group's whole
// 32-row tiles come from the epilogue's partials; a tile that a group boundary cuts gives the group its rows on this side of the
// boundary, re-read from z: (mean, M2) of the <= 31 rows in fp64, one row per segment through LDS — the head piece before the
// first whole tile, the tail piece after the last.  The last group owns the map's short last tile as a whole tile when it begins
// on or before that tile's first row.
__global__ __launch_bounds__(SCOLS * SSEG) void bn_stats_merge_groups_kernel(const float* __restrict__ part, int n_tiles, int n_rows, int C,
                                                                              float eps, float momentum, const float* __restrict__ z,
                                                                              int ld_z, const int* __restrict__ grp, int G,
                                                                              float* __restrict__ mean, float* __restrict__ invstd,
                                                                              float* __restrict__ rmean, float* __restrict__ rvar) {
  __shared__ double sh[3][SSEG][SCOLS];
  __shared__ float zs[SSEG][SCOLS];                                         // rows 0 .. 31 the head piece, 32 .. 63 the tail piece
  const int lc = threadIdx.x % SCOLS, seg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  for (int g = 0; g < G; ++g) {
    const int r0 = grp[g], r1 = grp[g + 1];
    if (r0 < 0 || r1 <= r0 || r1 > n_rows) continue;                      // uniform
    const int ta = (r0 + 31) >> 5;
    int tb = r1 == n_rows ? n_tiles : r1 >> 5;
    if (tb < ta) tb = ta;
    const int head0 = r0, head1 = (r0 & 31) ? min(r1, ta * 32) : r0;       // [head0, head1): before the first whole tile
    const int tail0 = (r1 != n_rows && (r1 & 31) && (r1 >> 5) >= ta) ? (r1 >> 5) * 32 : r1, tail1 = r1;
    {
      const int row = seg < 32 ? head0 + seg : tail0 + (seg - 32);
      const bool in = seg < 32 ? row < head1 : row < tail1;
      zs[seg][lc] = in ? z[(long long)row * ld_z + col] : 0.f;
    }
    double n = 0.0, mu = 0.0, m2 = 0.0;
    merge_tiles(n, mu, m2, part, ta, tb, n_rows, C, col, seg, lc, sh);
    if (seg == 0) {
      for (int piece = 0; piece < 2; ++piece) {
        const int cnt = piece ? tail1 - tail0 : head1 - head0, base = piece * 32;
        if (cnt <= 0) continue;
        double s = 0.0, d2 = 0.0;
        for (int r = 0; r < cnt; ++r) s += (double)zs[base + r][lc];
        const double pm = s / (double)cnt;
        for (int r = 0; r < cnt; ++r) { const double d = (double)zs[base + r][lc] - pm; d2 += d * d; }
        chan_merge(n, mu, m2, (double)cnt, pm, d2);
      }
      bn_finish(n, mu, m2, col, eps, momentum, mean + g * C, invstd + g * C, rmean, rvar);
    }
    __syncthreads();                                                      // segment 0 has read zs: the next group may write it
  }
}

struct BnSumsP {
  const double* part; int n_parts, M, C; long long n_rows;
  float* dgamma[MAXT]; float* dbeta[MAXT];
  float* coef;                                 // [G][1 + M][C], may be NULL
  const int* grp; int G;                       // GROUPED only
};

// sum of the parts [p0, p1) of quantity q (0 = sum g', 1 + m = sum g' xhat_m) for 16 columns: a thread adds its segment of that
// part list in part order, the 64 segments are added pairwise in a fixed tree.  Segment 0 has the sum: it writes its mean over
// the `count` rows as the coefficients of group g and adds it to tot (a sum that begins at +0.0 is never -0.0: 0.0 + s is s).
__device__ __forceinline__ void sums_span(const BnSumsP& p, int p0, int p1, long long count, int g, int q, int nq, int col, int seg,
                                          int lc, double (*sh)[SCOLS], double& tot) {
  const int per = (max(p1 - p0, 0) + SSEG - 1) / SSEG;
  const int t0 = p0 + seg * per, t1 = min(p1, t0 + per);
  double s = 0.0;
  for (int t = t0; t < t1; ++t) s += p.part[((long long)t * nq + q) * p.C + col];
  for (int stride = 1; stride < SSEG; stride <<= 1) {
    sh[seg][lc] = s;
    __syncthreads();
    if (seg % (2 * stride) == 0) s += sh[seg + stride][lc];
    __syncthreads();
  }
  // the total is added inside this branch and nq comes from the kernel: otherwise the kernel reads M again at its end
  if (seg == 0) {
    if (p.coef) p.coef[((long long)g * nq + q) * p.C + col] = (float)(s / (double)count);
    tot += s;
  }
}

// one quantity q (blockIdx.y) of 16 columns per work-group.  GROUPED: the parts of group g are consecutive; their sum gives the
// group's means (coef), and the groups' sums are added in ascending order for dgamma / dbeta
template <bool GROUPED>
__global__ __launch_bounds__(SCOLS * SSEG) void rows_bn_act_sums_kernel(const BnSumsP p) {
  __shared__ double sh[SSEG][SCOLS];
  const int lc = threadIdx.x % SCOLS, seg = threadIdx.x / SCOLS, col = blockIdx.x * SCOLS + lc;
  const int q = blockIdx.y, nq = 1 + p.M;
  double tot = 0.0;
  if constexpr (!GROUPED) {
    sums_span(p, 0, p.n_parts, p.n_rows, 0, q, nq, col, seg, lc, sh, tot);
  } else {
    for (int g = 0; g < p.G; ++g) {
      const long long a = (long long)p.grp[g], b = (long long)p.grp[g + 1];
      if (a < 0 || b <= a || b > p.n_rows) continue;                        // uniform
      const int p0 = max(part_index(p.grp, g, a >> 6), 0), p1 = min(part_index(p.grp, g, (b - 1) >> 6) + 1, p.n_parts);
      sums_span(p, p0, p1, b - a, g, q, nq, col, seg, lc, sh, tot);
    }
  }
  if (seg != 0) return;
#pragma unroll
  for (int m = 0; m < MAXT; ++m) {
    if (1 + m >= nq) continue;
    if (q == 0 && p.dbeta[m]) p.dbeta[m][col] = (float)tot;
    if (q == 1 + m && p.dgamma[m]) p.dgamma[m][col] = (float)tot;
  }
}

struct WsLayout { long long part, coef, total; };
WsLayout ws_layout(long long n_rows, int C, int M, int G) {
  WsLayout L{};
  long long o = 0;
  L.part = o; o += up256(((n_rows + 63) / 64 + G - 1) * (1 + M) * C * (long long)sizeof(double));
  L.coef = o; o += up256((long long)G * (1 + M) * C * (long long)sizeof(float));
  L.total = o;
  return L;
}


}  // namespace

long long csn_rows_bn_act_ws_bytes(long long n_rows, int C, int n_terms, int n_groups) {
  return ws_layout(n_rows, C, n_terms, n_groups).total;
}

int csn_launch_bn_stats_merge(const float* part, int n_tiles, int n_rows, int C, float eps, float momentum, const float* z, int ld_z,
                              const int* group_rows, int n_groups, float* mean, float* invstd, float* running_mean, float* running_var,
                              hipStream_t st) {
  if (group_rows)
    hipLaunchKernelGGL(bn_stats_merge_groups_kernel, dim3(C / SCOLS), dim3(SCOLS * SSEG), 0, st, part, n_tiles, n_rows, C, eps, momentum, z,
                       ld_z, group_rows, n_groups, mean, invstd, running_mean, running_var);
  else
    hipLaunchKernelGGL(bn_stats_merge_kernel, dim3(C / SCOLS), dim3(SCOLS * SSEG), 0, st, part, n_tiles, n_rows, C, eps, momentum, mean,
                       invstd, running_mean, running_var);
  return (int)hipGetLastError();
}

int csn_launch_rows_bn_act_fwd(const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, hipStream_t st) {
  const BnActP p = make_p(a, group_rows, n_groups);
  const unsigned n_chunks = (unsigned)(((long long)a.n_rows + 63) / 64);
  hipLaunchKernelGGL(group_rows ? rows_bn_act_groups_fwd_kernel : rows_bn_act_fwd_kernel, dim3(n_chunks), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// pass 1 or 2 of the backward on fp32 maps (the CsnBnActPass of csn_launch_rows_bn_act_bwd)
static int bwd_pass_f32(int pass, const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, double* part, const float* coef, int n_parts,
                        hipStream_t st) {
  BnActP p = make_p(a, group_rows, n_groups);
  p.part = part; p.coef = coef; p.n_parts = n_parts;
  const bool grouped = group_rows != nullptr;
  const int n_chunks = (int)(((long long)a.n_rows + 63) / 64);
  if (pass == 1)
    hipLaunchKernelGGL((grouped ? rows_bn_act_bwd_kernel<1, true> : rows_bn_act_bwd_kernel<1, false>), dim3(n_chunks), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((grouped ? rows_bn_act_bwd_kernel<2, true> : rows_bn_act_bwd_kernel<2, false>), dim3(n_chunks), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// pass 1, the sums, pass 2; `pass` launches the two row passes (NULL: the fp32 kernels of this file; train_maps16.hip hands over
// the passes that read y as bf16 rows, whole map only)
int csn_launch_rows_bn_act_bwd(const CsnRowsBnActArgs& a, const int* group_rows, int n_groups, hipStream_t st, CsnBnActPass pass) {
  if (!pass) pass = bwd_pass_f32;
  const bool grouped = group_rows != nullptr;
  const int G = grouped ? n_groups : 1;
  const WsLayout L = ws_layout(a.n_rows, a.C, a.n_terms, G);
  char* ws = static_cast<char*>(a.ws);
  double* part = reinterpret_cast<double*>(ws + L.part);
  float* coef = reinterpret_cast<float*>(ws + L.coef);
  const int n_chunks = (int)(((long long)a.n_rows + 63) / 64);
  const int n_parts = n_chunks + G - 1;
  bool any_dz = false, any_sum = false;
  for (int m = 0; m < a.n_terms; ++m) {
    any_dz |= a.dz[m] != nullptr;
    any_sum |= a.dgamma[m] != nullptr || a.dbeta[m] != nullptr;
  }
  const bool need_coef = any_dz && (a.training || grouped);                  // the grouped passes are training passes
  if (a.dr || any_sum || need_coef)
    if (const int e = pass(1, a, group_rows, n_groups, part, coef, n_parts, st)) return e;
  if (any_sum || need_coef) {
    BnSumsP s{};
    s.part = part; s.n_parts = n_parts; s.M = a.n_terms; s.C = a.C; s.n_rows = a.n_rows; s.coef = need_coef ? coef : nullptr;
    for (int m = 0; m < a.n_terms; ++m) { s.dgamma[m] = a.dgamma[m]; s.dbeta[m] = a.dbeta[m]; }
    s.grp = group_rows; s.G = G;
    hipLaunchKernelGGL(grouped ? rows_bn_act_sums_kernel<true> : rows_bn_act_sums_kernel<false>, dim3(a.C / SCOLS, 1 + a.n_terms),
                       dim3(SCOLS * SSEG), 0, st, s);
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (any_dz)
    if (const int e = pass(2, a, group_rows, n_groups, part, coef, n_parts, st)) return e;
  return 0;
}
