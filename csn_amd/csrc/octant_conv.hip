// Kernel-2 stride-2 convolution on voxel rows and its transposed form (MinkowskiNet/models/res16unet.py: conv1p1s2 .. conv4p8s2,
// convtr4p16s2 .. convtr7p2s2).  Kernel 2 at stride 2 PARTITIONS the fine voxels: every fine row i has one parent[i] among the
// coarse rows and sits in one octant[i] of it; children[8][n_coarse] is the inverse (-1: no voxel).  Two products follow:
//
//   gather form        y[j] = sum_k x[children[k][j]] B[k] (+ bias): the down convolution's forward (B = W) and the up convolution's
//                      input gradient (B[k] = W[k]^T).  This IS the gather-GEMM of sparse_conv.hip over a table of 8 offsets; its
//                      launchers are called as they are (csn_launch_sparse_conv_fwd / _bwd take any kv <= 125).
//   one-weight form    y[i] = x[parent[i]] B[octant[i]] (+ bias): the up convolution's forward and the down convolution's input
//                      gradient.  On the gather-GEMM a work-group's 128 sorted rows hold all 8 octants and 8 products are formed
//                      for each one used; here the rows are walked in `order` (sorted by octant, seg[9] the bounds) and a
//                      work-group's tile of <= 128 entries lies inside ONE segment: tiles are cut at the segment bounds, so the
//                      grid is ceil(n_fine / 128) + 7 row groups, and a work-group finds its (octant, range) from the 9 device
//                      integers (octant_span) and leaves when it has none.  A lane gathers the row parent[order[r]] through one
//                      buffer descriptor (rows_mma.h's row product, one W[k] for the whole tile) and the wave stores row order[r]:
//                      every output row exactly once, an empty segment costs nothing.
//   octant_wgrad       dw[k] = sum_{i : octant[i] = k} a_row(i)^T (x) dy_row(i): the weight gradient of rows_mma.h over the rows of
//                      segment k alone (work proportional to n_fine, not 8 n_fine).  Split-K over chunks of `order` cut at the
//                      segment bounds like the tiles; a chunk's four waves are added through LDS in wave order into the chunk's
//                      slab, and octant_slab_reduce adds an octant's slabs in chunk order (an empty octant's dw is written as 0).
//   dbias = sum of dy rows: csn_launch_rows_colsum / _merge (rows_fc.hip).
// Indices: a negative entry is "no voxel"; an entry past its array is dropped before it is used as an index, a gathered row goes
// through the buffer range check.  seg is clamped to a monotone sequence inside [0, n_fine], so no tile leaves `order` whatever
// seg holds.  No floating-point atomics: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

constexpr int TARGET_GROUPS = 256;      // as in sparse_conv.hip: work-groups a launch should offer before it is split finer

struct OctRowsP {
  const float* a; int lda; int n_src;   // A[n_src][lda]: the gathered (coarse) map
  const int* parent;                    // [M]
  const int* order;                     // [M] rows sorted by (octant, row)
  const int* seg;                       // [9]
  const float* b;                       // W[8][c_in][c_out]
  int c_in, c_out;
  float* c; int ldc;                    // C[M][ldc]
  int M, K, J;
  const float* bias;
};

// the inference epilogue's arguments on top of the product's (bias stays unused): c[order[r]] = act(acc * s + t + r[order[r]]),
// s = gamma / sqrt(rvar + eps), t = beta - rmean * s
struct OctRowsBnP : OctRowsP {
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps;
  const float* r; int ldr;              // residual [M][ldr], optional; may be c itself with ldr == ldc
  int relu;
};
// The epilogue's own arguments, read from the kernel-argument segment after the loop and not at kernel entry (bn_args_late of
// sparse_conv.hip: read at entry they would sit in scalar registers across the contraction loop).
typedef const OctRowsBnP __attribute__((address_space(4)))* OctRowsBnLateP;
__device__ __forceinline__ OctRowsBnLateP oct_bn_args_late() {
  OctRowsBnLateP k = (OctRowsBnLateP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// C[order[r]] = A[parent[order[r]]] * B[k] (+ bias) for the entries r of one tile of segment k.  B_KN: B[k] = W[k] ([K][J]), else
// W[k]^T (the same memory read [J][K]).  grid: column groups of NB * 32 fastest, then ceil(M / 128) + 7 row groups
// (BN is stated in terms of NB so that the body's choice between the two epilogues is made per instance, as in sparse_conv.hip)
template <int NB, int MODE, bool B_KN>
__global__ __launch_bounds__(256) void octant_rows_kernel(const OctRowsP p) {
  constexpr bool BN = NB < 0, STATS = NB < 0;
#include "octant_rows_body.inc"
}

// the up convolution's forward with the inference epilogue: the same body, kernels of their own (the instances above keep their
// names, arguments and code)
template <int NB, int MODE>
__global__ __launch_bounds__(256) void octant_rows_bn_kernel(const OctRowsBnP p) {
  constexpr bool B_KN = true, BN = NB > 0, STATS = NB < 0;
#include "octant_rows_body.inc"
}

struct OctWgradP {
  const float* a; int lda; int n_a;     // the rows that give dw's rows: [n_a][lda], c_in wide
  const float* b; int ldb; int n_b;     // the rows that give dw's columns: [n_b][ldb], c_out wide
  const int* parent; const int* order; const int* seg;
  int a_par;                            // 1: entry i reads a[parent[i]] and b[i] (up); 0: a[i] and b[parent[i]] (down)
  int n_fine, c_in, c_out, chunk;
  float* slabs;                         // [slot][c_in][c_out]
};

// grid: x = 64-column blocks of c_out, y = 32 TA-row blocks of c_in, z = ceil(n_fine / chunk) + 7 chunk slots
template <int TA, int MODE>
__global__ __launch_bounds__(256) void octant_wgrad_kernel(const OctWgradP p) {
  __shared__ float red[TA * WG_TB * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 32 * TA;
  int k, lo, hi;
  if (!octant_span(p.seg, p.n_fine, (int)blockIdx.z, p.chunk, k, lo, hi)) return;   // uniform over the work-group
  const int nbv = (p.c_out - co0) >= 64 ? 2 : 1;                      // column blocks of b inside c_out (c_out % 32 == 0)
  const int quarter = p.chunk >> 2;                                   // chunk % 64 == 0
  const int rb = lo + wave * quarter;
  const long long left = (long long)hi - rb;
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_a - 1) * p.lda + p.c_in) * 4LL);
  const csn_rsrc_t br = csn_make_rsrc(p.b, ((long long)(p.n_b - 1) * p.ldb + p.c_out) * 4LL);

  f32x16 acc[TA][WG_TB] = {};
  float an[TA][8], bn[WG_TB][8];
  auto load = [&](int rr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + wgrad_row<MODE>(h, e);
      int i = row < left ? p.order[rb + row] : -1;
      if (i >= p.n_fine) i = -1;
      const int par = i >= 0 ? p.parent[i] : -1;
      const int ia = p.a_par ? par : i, ib = p.a_par ? i : par;
      const bool ok = ia >= 0 && ia < p.n_a && ib >= 0 && ib < p.n_b;
      const unsigned ao = ok ? ((unsigned)ia * (unsigned)p.lda + (unsigned)(ci0 + li)) * 4u : CSN_OOB;
      const unsigned bo = ok ? ((unsigned)ib * (unsigned)p.ldb + (unsigned)(co0 + li)) * 4u : CSN_OOB;
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) an[ta][e] = csn_bload(ar, ao + (unsigned)(ta * 128));
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bn[tb][e] = tb < nbv ? csn_bload(br, bo + (unsigned)(tb * 128)) : 0.f;
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
    wgrad_step<TA, MODE, true>(acc, af, bf, nbv);
  }
  wgrad_reduce_store<TA>(acc, red, p.slabs + (long long)blockIdx.z * p.c_in * p.c_out, p.c_out, ci0, co0, nbv, wave, l);
}

// dw[k] = the slabs of octant k's chunk slots added in slot order (0 where it has none).  grid: x = n / 1024, y = 8 octants
__global__ __launch_bounds__(256) void octant_slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                                 const int* __restrict__ seg, int n_fine, int chunk, long long n) {
  const int k = blockIdx.y;
  int s0 = min(max(seg[0], 0), n_fine), t0 = 0, cnt = 0;
  for (int kk = 0; kk <= k; ++kk) {
    const int s1 = min(max(seg[kk + 1], s0), n_fine);
    t0 += cnt;
    cnt = (s1 - s0 + chunk - 1) / chunk;
    s0 = s1;
  }
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  for (int t = t0; t < t0 + cnt; ++t) sum += *reinterpret_cast<const f32x4*>(slabs + (long long)t * n + e);
  *reinterpret_cast<f32x4*>(dw + (long long)k * n + e) = sum;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline int wgrad_ta_for(int c_in) {
  const int t = c_in / 32;
  return t % 4 == 0 ? 4 : (t % 3 == 0 ? 3 : (t % 2 == 0 ? 2 : 1));
}

// split-K of the weight gradient: about one work-group per CU over (tile, chunk); chunks of a multiple of 64 rows
int wgrad_chunk(long long n_fine, int c_in, int c_out) {
  const long long tiles = (long long)((c_out + 63) / 64) * (c_in / (32 * wgrad_ta_for(c_in)));
  const long long want = (TARGET_GROUPS + tiles - 1) / tiles;
  long long ch = ((n_fine + want - 1) / want + 63) / 64 * 64;
  if (ch > 65536) ch = 65536;
  return (int)ch;
}
inline long long wgrad_slots(long long n_fine, int chunk) { return (n_fine + chunk - 1) / chunk + 7; }

struct WsLayout { long long part, slabs, total; };

// n_dy: the rows of dy (the coarse rows of the down convolution, the fine rows of the up convolution)
WsLayout ws_layout(long long n_fine, long long n_dy, int c_in, int c_out) {
  WsLayout L{};
  long long o = 0;
  L.part = o;  o += up256(((n_dy + 63) / 64) * c_out * (long long)sizeof(double));
  L.slabs = o; o += up256(wgrad_slots(n_fine, wgrad_chunk(n_fine, c_in, c_out)) * c_in * c_out * (long long)sizeof(float));
  L.total = o;
  return L;
}

template <int NB, bool B_KN>
int launch_rows_nb(const OctRowsP& p, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128 + 7);
  if (groups > 0x7fffffffLL) return -5;
  auto* const k = mode == 0 ? octant_rows_kernel<NB, 0, B_KN> : octant_rows_kernel<NB, 1, B_KN>;
  hipLaunchKernelGGL(k, dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// the instances with the inference epilogue (the up convolution's forward only)
template <int NB, bool B_KN>
int launch_rows_nb(const OctRowsBnP& p, int mode, hipStream_t st) {
  static_assert(B_KN, "the inference epilogue belongs to the forward product");
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128 + 7);
  if (groups > 0x7fffffffLL) return -5;
  auto* const k = mode == 0 ? octant_rows_bn_kernel<NB, 0> : octant_rows_bn_kernel<NB, 1>;
  hipLaunchKernelGGL(k, dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// the column blocks a wave owns (csn_octant_column_blocks below)
template <bool B_KN, typename P>
int launch_rows(const P& p, int mode, hipStream_t st) {
  return dispatch4(csn_octant_column_blocks(p.J, p.M), [&](auto n) { return launch_rows_nb<n(), B_KN>(p, mode, st); });
}

template <int TA>
int launch_wgrad_ta(const OctWgradP& p, int slots, int mode, hipStream_t st) {
  const dim3 grid((unsigned)((p.c_out + 63) / 64), (unsigned)(p.c_in / (32 * TA)), (unsigned)slots);
  auto* const k = mode == 0 ? octant_wgrad_kernel<TA, 0> : octant_wgrad_kernel<TA, 1>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// dw and dbias of either direction; a / b as in OctWgradP
int launch_wgrad(const CsnOctantConvArgs& a, bool up, hipStream_t st, int mode) {
  const long long n_dy = up ? a.n_fine : a.n_coarse;
  const WsLayout L = ws_layout(a.n_fine, n_dy, a.c_in, a.c_out);
  char* ws = static_cast<char*>(a.ws);
  if (a.dbias) {
    double* part = reinterpret_cast<double*>(ws + L.part);
    if (const int e = csn_launch_rows_colsum(a.dy, a.ld_dy, n_dy, a.c_out, part, st)) return e;
    if (const int e = csn_launch_rows_colsum_merge(part, (int)((n_dy + 63) / 64), a.c_out, a.dbias, st)) return e;
  }
  if (a.dw) {
    OctWgradP p{};
    p.a = a.x; p.lda = a.ld_x; p.n_a = up ? a.n_coarse : a.n_fine;
    p.b = a.dy; p.ldb = a.ld_dy; p.n_b = (int)n_dy;
    p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.a_par = up;
    p.n_fine = a.n_fine; p.c_in = a.c_in; p.c_out = a.c_out; p.chunk = wgrad_chunk(a.n_fine, a.c_in, a.c_out);
    p.slabs = reinterpret_cast<float*>(ws + L.slabs);
    const int slots = (int)wgrad_slots(a.n_fine, p.chunk);
    if (const int e = dispatch4(wgrad_ta_for(a.c_in), [&](auto ta) { return launch_wgrad_ta<ta()>(p, slots, mode, st); })) return e;
    const long long n = (long long)a.c_in * a.c_out;
    hipLaunchKernelGGL(octant_slab_reduce_kernel, dim3((unsigned)(n / 1024), 8), dim3(256), 0, st, p.slabs, a.dw, a.seg, a.n_fine,
                       p.chunk, n);
    return (int)hipGetLastError();
  }
  return 0;
}

// the gather form on sparse_conv.hip's launchers: children[8][n_coarse] is a kernel map of 8 offsets
CsnSparseConvArgs gather_args(const CsnOctantConvArgs& a) {
  CsnSparseConvArgs g{};
  g.kv = 8; g.c_in = a.c_in; g.c_out = a.c_out; g.w = a.w;
  return g;
}

}  // namespace

// the column blocks a wave owns in a one-weight product of J columns over M rows: the rule of sparse_conv.hip's launch_gemm
// (CSN_DEV_SCONV_NB pins them here too); octant_conv_maps16.hip launches by it as well
int csn_octant_column_blocks(int J, long long M) {
  const int t = J / 32;
  int nb = t <= 4 ? t : (t + 1) / 2;
  const long long row_groups = (M + 127) / 128;
  while (nb > 1 && row_groups * ((t + nb - 1) / nb) < TARGET_GROUPS) nb = (nb + 1) / 2;
  if (csn_dev_sconv_nb > 0) nb = csn_dev_sconv_nb < t ? csn_dev_sconv_nb : t;
  return nb;
}

long long csn_octant_conv_ws_bytes(long long n_fine, long long n_coarse, int c_in, int c_out, int up, int backward) {
  return backward ? ws_layout(n_fine, up ? n_fine : n_coarse, c_in, c_out).total : 0;
}

// mode: 0 fp32, anything else bf16x3 (the single-product forwards of section 25 are octant_conv_maps16.hip)
int csn_launch_octant_down_fwd(const CsnOctantConvArgs& a, int mode, hipStream_t st) {
  CsnSparseConvArgs g = gather_args(a);
  g.x = a.x; g.ld_x = a.ld_x; g.n_in = a.n_fine; g.fwd_table = a.children; g.n_out = a.n_coarse; g.bias = a.bias; g.y = a.y; g.ld_y = a.ld_y;
  return csn_launch_sparse_conv_fwd(g, mode != 0, st);
}

int csn_launch_octant_down_bwd(const CsnOctantConvArgs& a, int mode, hipStream_t st) {
  if (a.dx) {
    // dx[i] = dy[parent[i]] W[octant[i]]^T: contraction over c_out
    OctRowsP p{};
    p.a = a.dy; p.lda = a.ld_dy; p.n_src = a.n_coarse; p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.b = a.w;
    p.c_in = a.c_in; p.c_out = a.c_out; p.c = a.dx; p.ldc = a.ld_dx; p.M = a.n_fine; p.K = a.c_out; p.J = a.c_in;
    if (const int e = launch_rows<false>(p, mode != 0, st)) return e;
  }
  return launch_wgrad(a, false, st, mode != 0);
}

int csn_launch_octant_up_fwd(const CsnOctantConvArgs& a, int mode, hipStream_t st) {
  OctRowsP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_coarse; p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.b = a.w;
  p.c_in = a.c_in; p.c_out = a.c_out; p.c = a.y; p.ldc = a.ld_y; p.M = a.n_fine; p.K = a.c_in; p.J = a.c_out; p.bias = a.bias;
  return launch_rows<true>(p, mode != 0, st);
}

// the two forwards with the inference epilogue (include/csn_hip.h section 23): one launch each, no workspace.  Down is the
// gather-GEMM's BN instances over children[8][n_coarse]; a coarse row without children has acc = 0 and gives act(t + r)
int csn_launch_octant_down_bn_act_fwd(const CsnOctantConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  CsnSparseConvArgs g = gather_args(a);
  g.x = a.x; g.ld_x = a.ld_x; g.n_in = a.n_fine; g.fwd_table = a.children; g.n_out = a.n_coarse; g.y = a.y; g.ld_y = a.ld_y;
  return csn_launch_sparse_conv_bn_act_fwd(g, n, mode != 0, st);
}

int csn_launch_octant_up_bn_act_fwd(const CsnOctantConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  OctRowsBnP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_coarse; p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.b = a.w;
  p.c_in = a.c_in; p.c_out = a.c_out; p.c = a.y; p.ldc = a.ld_y; p.M = a.n_fine; p.K = a.c_in; p.J = a.c_out;
  p.gamma = n.gamma; p.beta = n.beta; p.rmean = n.running_mean; p.rvar = n.running_var; p.eps = n.eps;
  p.r = n.r; p.ldr = n.ld_r; p.relu = n.relu;
  return launch_rows<true>(p, mode != 0, st);
}

int csn_launch_octant_up_bwd(const CsnOctantConvArgs& a, int mode, hipStream_t st) {
  if (a.dx) {
    // dx[j] = sum_k dy[children[k][j]] W[k]^T: the gather-GEMM's input gradient with children as its second table
    CsnSparseConvArgs g = gather_args(a);
    g.dy = a.dy; g.ld_dy = a.ld_dy; g.n_out = a.n_fine; g.bwd_table = a.children; g.n_in = a.n_coarse; g.dx = a.dx; g.ld_dx = a.ld_dx;
    if (const int e = csn_launch_sparse_conv_bwd(g, mode != 0, st)) return e;
  }
  return launch_wgrad(a, true, st, mode != 0);
}
