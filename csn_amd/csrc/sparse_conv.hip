// Sparse 3D convolution on voxel rows (MinkowskiNet/models/hrnet.py:39-53, 89-111, 233-239; models/modules/resnet_block.py:22-57):
// kernel 3 / 5 at stride 1, kernel 3 at stride 2 and its transposed form are ONE gather-GEMM over a kernel map
// table[KV][n_out] (int32: the source row of output row j at offset k, or -1) — forward and backward.
//
//   sconv_gemm         C[j] = sum_k A[table[k][j]] * B[k] (+ bias).  The row product of rows_mma.h with a lane's row address looked
//                      up per offset: a lane owns one output row and reads 4 / 8 consecutive channels of its source row through one
//                      buffer descriptor over the whole source map; a -1 entry (and a row past the end) gives the lane CSN_OOB, so
//                      it reads zeros — no lane mask around the matrix instructions.  The contraction runs over (offset,
//                      32-channel step); each W[k] step is staged through LDS once per work-group.  An offset at which no row of
//                      the work-group's 128-row tile has a neighbour is dropped from the work-group's offset list before the loop
//                      (wave ballots, merged through LDS: uniform over the work-group).  Forward: A = x, table = fwd, B[k] =
//                      W[k] ([c_in][c_out], B_KN).  dx: A = dy, table = bwd, B[k] = W[k]^T (the same memory read [J][K]).
//                      Every output row is written by exactly one wave.  With a partials pointer the epilogue also forms the
//                      (mean, M2) of each wave's <= 32 rows from the accumulators (the BatchNorm statistics of the backbone's
//                      convolutions, csn_sparse_conv_stats_fwd_f32); the stored values are the same bits either way.
//                      The BN forward instances (csn_sparse_conv_bn_act_fwd_f32, inference) store act(acc * s + t + r) instead:
//                      a BatchNorm on its running statistics, an optional residual and the ReLU in the product's epilogue.
//   sconv_wgrad        dW[k][ci][co] = sum_j x[fwd[k][j]][ci] dy[j][co] over the output rows of one split-K chunk: the weight
//                      gradient of rows_mma.h with one gathered operand (a lane's 8 contraction steps are 8 looked-up rows of one column: a half wave
//                      reads one contiguous 128-byte run per row).  A 16-row step in which the wave finds no neighbour is skipped
//                      (wave ballot).  The four waves contract a quarter of the chunk each and are added through LDS in wave
//                      order; the chunks are slabs added in order by csn_launch_slab_reduce.
//   dbias = sum_j dy[j]: csn_launch_rows_colsum / _merge (rows_fc.hip), fp64 sums of 64-row chunks added in chunk order.
//   sconv_gemm16 / sconv_wgrad16   the same bodies with ONE 16-bit product per operand pair (math modes 2 bf16 / 3 fp16 behind
//                      csn_set_thread_rows16; fp16: the forward alone): operands rounded once, W converted when it is stored to LDS.
// No floating-point atomics anywhere: every reduction has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

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
  float* part;                         // non-NULL: the (mean, M2) of each wave's rows, [tile][2][J], tile = 32 rows
};

// the inference epilogue's arguments on top of the product's (bias and part stay unused): y = act(acc * s + t + r),
// s = gamma / sqrt(rvar + eps), t = beta - rmean * s
struct SconvBnP : SconvGemmP {
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps;
  const float* r; int ldr;             // residual [M][ldr], optional; may be c itself with ldr == ldc
  int relu;
};
// The epilogue's own arguments, read from the kernel-argument segment (the by-value argument is its first and only entry) at the
// point of the call instead of at kernel entry, where the compiler reads a by-value argument: read there they stay in scalar
// registers across the contraction loop, the NB >= 2 instances have none to spare, 16 of them spill into vector registers and the
// fp32 NB = 4 instance (105 + 64 accumulator registers) loses a wave per SIMD.  The empty asm keeps the reads below it.
typedef const SconvBnP __attribute__((address_space(4)))* SconvBnLateP;
__device__ __forceinline__ SconvBnLateP bn_args_late() {
  SconvBnLateP k = (SconvBnLateP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// (BN is stated in terms of NB so that the body's choice between the two epilogues is made per instance: the epilogue an
// instance does not take is never instantiated for its argument type)
template <int NB, int MODE, bool B_KN>
__global__ __launch_bounds__(256) void sconv_gemm_kernel(const SconvGemmP p) {
  constexpr bool BN = NB < 0, ACC = false;
#include "sconv_gemm_body.inc"
}

// the single-product instances: H16 = fp16 operands (forward only), else bf16
template <int NB, bool H16, bool B_KN>
__global__ __launch_bounds__(256) void sconv_gemm16_kernel(const SconvGemmP p) {
  constexpr int MODE = H16 ? 3 : 2;
  constexpr bool BN = NB < 0, ACC = false;
#include "sconv_gemm_body.inc"
}

// the forward instances with the inference epilogue: the same body, kernels of their own (the instances above keep their names,
// arguments and code)
template <int NB, int MODE>
__global__ __launch_bounds__(256) void sconv_gemm_bn_kernel(const SconvBnP p) {
  constexpr bool B_KN = true, BN = NB > 0, ACC = false;
#include "sconv_gemm_body.inc"
}

template <int NB, bool H16>
__global__ __launch_bounds__(256) void sconv_gemm16_bn_kernel(const SconvBnP p) {
  constexpr int MODE = H16 ? 3 : 2;
  constexpr bool B_KN = true, BN = NB > 0, ACC = false;
#include "sconv_gemm_body.inc"
}

// dW[k][ci][co] = sum_j x[fwd[k][j]][ci] dy[j][co] over the rows of one split-K chunk; see the file header.
// grid: x = 64-column blocks of c_out, y = 32 TA-row blocks of c_in, z = KV * splits (offset fastest)
// the body of sconv_wgrad_kernel (MODE 0 / 1) and sconv_wgrad16_kernel (MODE 2: one bf16 product)
template <int TA, int MODE>
__device__ __forceinline__ void sconv_wgrad_body(const float* __restrict__ x, int ldx, int n_in, const int* __restrict__ table,
                                                 const float* __restrict__ dy, int ldy, float* __restrict__ out, int n_out, int c_in,
                                                 int c_out, int KV, int chunk) {
  __shared__ float red[TA * WG_TB * 16 * 64];
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

  f32x16 acc[TA][WG_TB] = {};
  float an[TA][8], bn[WG_TB][8];
  int src[8];
  // the source rows of step st; returns whether any lane of the wave found one
  auto lookup = [&](int rr) -> bool {
    bool any = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + wgrad_row<MODE>(h, e);
      src[e] = row < left ? tbl[row] : -1;
      any |= src[e] >= 0;
    }
    return __ballot(any) != 0ULL;
  };
  auto load = [&](int rr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = rr + wgrad_row<MODE>(h, e);
      const unsigned xo = src[e] < 0 ? CSN_OOB : ((unsigned)src[e] * (unsigned)ldx + (unsigned)(ci0 + li)) * 4u;
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) an[ta][e] = csn_bload(xr, xo + (unsigned)(ta * 128));
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
    float af[TA][8], bf[WG_TB][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int ta = 0; ta < TA; ++ta) af[ta][e] = an[ta][e];
#pragma unroll
      for (int tb = 0; tb < WG_TB; ++tb) bf[tb][e] = bn[tb][e];
    }
    any_n = false;
    if (st + 1 < n_steps) {
      any_n = lookup((st + 1) * 16);
      if (any_n) load((st + 1) * 16);
    }
    if (!any_c) continue;                                             // wave-uniform: no neighbour at this offset in these 16 rows
    wgrad_step<TA, MODE, true>(acc, af, bf, nbv);
  }
  wgrad_reduce_store<TA>(acc, red, out + ((long long)split * KV + kv) * c_in * c_out, c_out, ci0, co0, nbv, wave, l);
}

template <int TA, int MODE>
__global__ __launch_bounds__(256) void sconv_wgrad_kernel(const float* __restrict__ x, int ldx, int n_in, const int* __restrict__ table,
                                                          const float* __restrict__ dy, int ldy, float* __restrict__ out, int n_out,
                                                          int c_in, int c_out, int KV, int chunk) {
  sconv_wgrad_body<TA, MODE>(x, ldx, n_in, table, dy, ldy, out, n_out, c_in, c_out, KV, chunk);
}

template <int TA>
__global__ __launch_bounds__(256) void sconv_wgrad16_kernel(const float* __restrict__ x, int ldx, int n_in, const int* __restrict__ table,
                                                            const float* __restrict__ dy, int ldy, float* __restrict__ out, int n_out,
                                                            int c_in, int c_out, int KV, int chunk) {
  sconv_wgrad_body<TA, 2>(x, ldx, n_in, table, dy, ldy, out, n_out, c_in, c_out, KV, chunk);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
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
  // the fp16 product exists for the forward (B_KN) alone
  void (*const k[4])(SconvGemmP) = {sconv_gemm_kernel<NB, 0, B_KN>, sconv_gemm_kernel<NB, 1, B_KN>, sconv_gemm16_kernel<NB, false, B_KN>,
                                    B_KN ? sconv_gemm16_kernel<NB, true, true> : nullptr};
  return launch_row_product(k, p, NB, mode, st);
}

// the instances with the inference epilogue (forward only)
template <int NB, bool B_KN>
int launch_gemm_nb(const SconvBnP& p, int mode, hipStream_t st) {
  static_assert(B_KN, "the inference epilogue belongs to the forward product");
  void (*const k[4])(SconvBnP) = {sconv_gemm_bn_kernel<NB, 0>, sconv_gemm_bn_kernel<NB, 1>, sconv_gemm16_bn_kernel<NB, false>,
                                  sconv_gemm16_bn_kernel<NB, true>};
  return launch_row_product(k, p, NB, mode, st);
}

// the wave owns every column up to 128; wider outputs take two column groups of the smallest width that covers them.  Where
// that leaves fewer than TARGET_GROUPS work-groups (the coarse levels: few rows, wide rows), the column groups are halved
// until it does not: more work-groups gather the same rows (from L2), each contracts a narrower slice.  The sums are the same.
// csn_dev_set(CSN_DEV_SCONV_NB, 1..4) pins the column blocks per wave instead (tests reach every instance at small sizes).
template <bool B_KN, typename P>
int launch_gemm(const P& p, int mode, hipStream_t st) {
  return dispatch4(csn_sconv_column_blocks(p.J, p.M), [&](auto n) { return launch_gemm_nb<n(), B_KN>(p, mode, st); });
}

template <int TA>
int launch_wgrad_ta(const CsnSparseConvArgs& a, float* out, int splits, int chunk, int mode, hipStream_t st) {
  const dim3 grid((unsigned)((a.c_out + 63) / 64), (unsigned)(a.c_in / (32 * TA)), (unsigned)(splits * a.kv)), block(256);
  auto* const k = mode == 0 ? sconv_wgrad_kernel<TA, 0> : (mode == 1 ? sconv_wgrad_kernel<TA, 1> : sconv_wgrad16_kernel<TA>);
  hipLaunchKernelGGL(k, grid, block, 0, st, a.x, a.ld_x, a.n_in, a.fwd_table, a.dy, a.ld_dy, out, a.n_out, a.c_in, a.c_out, a.kv, chunk);
  return (int)hipGetLastError();
}

}  // namespace

int csn_dev_sconv_nb = 0;

// launch_gemm's rule, stated once for every file that launches this product (sparse_conv_maps16.hip)
int csn_sconv_column_blocks(int J, long long M) {
  const int t = J / 32;
  int nb = t <= 4 ? t : (t + 1) / 2;
  const long long row_groups = (M + 127) / 128;
  while (nb > 1 && row_groups * ((t + nb - 1) / nb) < TARGET_GROUPS) nb = (nb + 1) / 2;
  if (csn_dev_sconv_nb > 0) nb = csn_dev_sconv_nb < t ? csn_dev_sconv_nb : t;
  return nb;
}

void csn_sconv_wgrad_plan(long long n_out, int kv, int c_in, int c_out, int* ta, int* splits, int* chunk, long long* slabs_offset) {
  *ta = wgrad_ta_for(c_in);
  wgrad_split(n_out, kv, c_in, c_out, *splits, *chunk);
  *slabs_offset = ws_layout(n_out, kv, c_in, c_out).slabs;
}

long long csn_sparse_conv_ws_bytes(long long n_in, long long n_out, int kv, int c_in, int c_out, int backward) {
  (void)n_in;
  return backward ? ws_layout(n_out, kv, c_in, c_out).total : 0;
}

// mode: 0 fp32, 1 bf16x3, 2 bf16 / 3 fp16 single product (csn_capi.hip resolves the thread's math mode and rows16 flag)
int csn_launch_sparse_conv_fwd(const CsnSparseConvArgs& a, int mode, hipStream_t st) {
  SconvGemmP p{};
  // w_rows: the rows of every W[k] where the contraction takes a slice [c0, c0 + c_in) of them (a.w points at row c0 of W[0])
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.w_rows ? a.w_rows : a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv; p.bias = a.bias;
  return launch_gemm<true>(p, mode, st);
}

// the forward product with the inference epilogue: one launch, no workspace
int csn_launch_sparse_conv_bn_act_fwd(const CsnSparseConvArgs& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  SconvBnP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv;
  p.gamma = n.gamma; p.beta = n.beta; p.rmean = n.running_mean; p.rvar = n.running_var; p.eps = n.eps;
  p.r = n.r; p.ldr = n.ld_r; p.relu = n.relu;
  return launch_gemm<true>(p, mode, st);
}

long long csn_sparse_conv_stats_ws_bytes(long long n_out, int c_out) {
  return up256(((n_out + 127) / 128) * 4 * 2 * c_out * (long long)sizeof(float));
}

// the forward product with the statistics epilogue, then the tiles' (mean, M2) merged in fp64 in a fixed order (rows_bn_act.hip).
// (20a) group_rows: the map's rows are n_groups BatchNorm batches — the same product and epilogue, the tiles merged per group
int csn_launch_sparse_conv_stats_fwd(const CsnSparseConvArgs& a, const int* group_rows, int n_groups, float* mean, float* invstd,
                                     float* running_mean, float* running_var, float eps, float momentum, int mode, hipStream_t st) {
  SconvGemmP p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.fwd_table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv; p.bias = nullptr;
  p.part = static_cast<float*>(a.ws);
  if (const int e = launch_gemm<true>(p, mode, st)) return e;
  const int n_tiles = (int)(((long long)a.n_out + 127) / 128) * 4;
  return csn_launch_bn_stats_merge(p.part, n_tiles, a.n_out, a.c_out, eps, momentum, a.y, a.ld_y, group_rows, n_groups, mean, invstd,
                                   running_mean, running_var, st);
}

int csn_launch_sparse_conv_bwd(const CsnSparseConvArgs& a, int mode, hipStream_t st) {
  if (mode == 3) return -1;                                           // fp16 is forward only
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
    if (const int e = csn_launch_rows_colsum(a.dy, a.ld_dy, a.n_out, a.c_out, part, st)) return e;
    if (const int e = csn_launch_rows_colsum_merge(part, (int)(((long long)a.n_out + 63) / 64), a.c_out, a.dbias, st)) return e;
  }
  if (a.dw) {
    int splits, chunk;
    wgrad_split(a.n_out, a.kv, a.c_in, a.c_out, splits, chunk);
    float* out = splits > 1 ? reinterpret_cast<float*>(ws + L.slabs) : a.dw;
    const int e = dispatch4(wgrad_ta_for(a.c_in), [&](auto ta) { return launch_wgrad_ta<ta()>(a, out, splits, chunk, mode, st); });
    if (e) return e;
    if (splits > 1) return csn_launch_slab_reduce(out, a.dw, splits, (long long)a.kv * a.c_in * a.c_out, 1.f, 0, st);
  }
  return 0;
}
