// The inference octant products of octant_conv.hip as ONE 16-bit product on 16-bit maps (include/csn_hip.h section 25): math modes
// 2 bf16 / 3 fp16 behind csn_set_thread_rows16, the BatchNorm + residual + ReLU epilogue of section 23, where the gathered map x,
// the residual r and the output y may each be rows of the mode's 16-bit type instead of fp32.
//
//   down               the gather form over children[8][n_coarse]: sparse_conv_maps16.hip's launcher as it is (a table of 8 offsets),
//                      the way section 23 reaches section 19's.  No kernel of its own.
//   octant_rows_m16_kernel<NB, H16, A16>   up: the walk of octant_rows_body.inc — tiles of <= 128 entries of `order` cut at the
//                      segment bounds (octant_span), one W[k] per tile, ceil(M / 128) + 7 row groups — with the tile of W staged as
//                      shorts (rounded when it is stored to LDS) and one matrix instruction per (half step, column block) in
//                      mma_step_a16's order.  A16: the parent row holds 16-bit values; a lane's two fragments of a 32-channel step
//                      are two 16-byte buffer loads at src * ld * 2 + s * 64 + 16 h and + 32 (no conversion).  !A16: the four
//                      loads and conversions of the fp32 single-product instances (mma_step<NB, MODE>).
//   epilogue           accumulator row e of the lane goes to row s_dst[..]: v = fma(acc, s, t) (+ r), ReLU; r is read as fp32 or
//                      as 16-bit elements (converted exactly), y is stored as fp32 or as to16(v): ONE rounding to nearest even, an
//                      fp16 overflow a plain conversion (inf).  32 lanes write one 128-byte or 64-byte run.  The two types are
//                      wave-uniform runtime flags (NB x mode x A type = 16 instances); every access goes through a buffer descriptor
//                      sized in bytes of the map's own type.  Each element of r is read and then written by the same lane: r may be y.
// Index rules as in octant_conv.hip: a destination outside [0, M) is dropped, a parent past n_src reads zeros, seg is clamped to a
// monotone sequence, every output row is written exactly once.  No workspace, no atomics: two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

struct OctM16P {
  const void* a; int lda; int n_src;   // A[n_src][lda]: the gathered (coarse) map, fp32 or 16-bit rows (the kernel's A16)
  const int* parent;                   // [M]
  const int* order;                    // [M] rows sorted by (octant, row)
  const int* seg;                      // [9]
  const float* b;                      // W[8][c_in][c_out]
  int c_in, c_out;
  void* c; int ldc;                    // C[M][ldc], fp32 or 16-bit rows (y16)
  int M, K, J;
  // the epilogue's arguments, read late (oct_m16_args_late)
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps;
  const void* r; int ldr;              // residual [M][ldr], optional, fp32 or 16-bit rows (r16); may be c itself, same type and pitch
  int relu, r16, y16;
};
// As oct_bn_args_late of octant_conv.hip: read from the kernel-argument segment after the loop, not held in scalar registers across it.
typedef const OctM16P __attribute__((address_space(4)))* OctM16LateP;
__device__ __forceinline__ OctM16LateP oct_m16_args_late() {
  OctM16LateP k = (OctM16LateP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// grid: column groups of NB * 32 fastest, then ceil(M / 128) + 7 row groups
template <int NB, bool H16, bool A16>
__global__ __launch_bounds__(256) void octant_rows_m16_kernel(const OctM16P p) {
  constexpr int MODE = H16 ? 3 : 2;
  __shared__ __attribute__((aligned(16))) short Bs[NB * 32 * BS16_PITCH];
  __shared__ int s_dst[128];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  int k, lo, hi;
  if (!octant_span(p.seg, p.M, rg, 128, k, lo, hi)) return;           // uniform over the work-group
  const int r = lo + wave * 32 + li;                                  // the lane's entry of `order`
  int dst = r < hi ? p.order[r] : -1;
  if (dst >= p.M) dst = -1;
  int src = dst >= 0 ? p.parent[dst] : -1;
  if (src >= p.n_src) src = -1;
  if (h == 0) s_dst[wave * 32 + li] = dst;
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * (A16 ? 2LL : 4LL));
  // the lane's channels inside a 32-channel step: bytes 16 h (+ 32) of its 64, or 32 h of its 128
  const unsigned a_row = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * (A16 ? 2u : 4u) + (unsigned)(A16 ? 16 * h : 32 * h);
  const float* bk = p.b + (long long)k * p.c_in * p.c_out;
  const int S = p.K >> 5;                                             // 32-channel steps

  f32x16 acc[NB] = {};
  constexpr int NA = A16 ? 2 : 4;                                     // 16-byte reads of A per lane and step
  f32x4 an[NA], bn[NB];
  auto load = [&](int s) {
    if constexpr (A16) {
      const unsigned off = src < 0 ? CSN_OOB : a_row + (unsigned)(s * 64);
      an[0] = csn_bload4(ar, off);
      an[1] = csn_bload4(ar, off + 32u);
    } else {
      const unsigned off = src < 0 ? CSN_OOB : a_row + (unsigned)(s * 128);
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, off + (unsigned)(a_kofs<MODE>(g) * 4));
    }
    load_b<NB, true>(bn, bk, p.c_out, s * 32, j0, p.J, tid);
  };
  load(0);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, true, MODE>(Bs, bn, tid);
    f32x4 af[NA];
#pragma unroll
    for (int g = 0; g < NA; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) load(s + 1);
    if constexpr (A16) mma_step_a16<NB, H16>(acc, af, Bs, li, h);
    else mma_step<NB, MODE>(acc, af, Bs, li, h);
  }

  // the wave's 32 rows leave for their own places: accumulator row e of the lane goes to row s_dst[..], 32 lanes one run of 128
  // (fp32) or 64 (16-bit) bytes
  const auto* q = oct_m16_args_late();
  const bool r16 = q->r16 != 0, y16 = q->y16 != 0;                     // wave-uniform
  const unsigned ysz = y16 ? 2u : 4u, rsz = r16 ? 2u : 4u;
  const csn_rsrc_t cr = csn_make_rsrc(p.c, ((long long)(p.M - 1) * p.ldc + p.J) * (long long)ysz);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    const int col = j0 + nb * 32 + li;
    const float sc = q->gamma[col] / sqrtf(q->rvar[col] + q->eps);
    const float sh = q->beta[col] - q->rmean[col] * sc;
    const void* rp = q->r;
    const int ldr = q->ldr;
    const bool relu = q->relu != 0;
    const csn_rsrc_t rr = csn_make_rsrc(rp, rp ? ((long long)(p.M - 1) * ldr + p.J) * (long long)rsz : 0LL);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int d = s_dst[wave * 32 + csn_acc_row(e, h)];
      float v = fmaf(acc[nb][e], sc, sh);
      if (rp) {
        const unsigned ro = d < 0 ? CSN_OOB : ((unsigned)d * (unsigned)ldr + (unsigned)col) * rsz;
        v += r16 ? from16<H16>(csn_bload16(rr, ro)) : csn_bload(rr, ro);
      }
      v = relu ? fmaxf(0.f, v) : v;
      const unsigned co = d < 0 ? CSN_OOB : ((unsigned)d * (unsigned)p.ldc + (unsigned)col) * ysz;
      if (y16) csn_bstore16(to16<H16>(v), cr, co);
      else csn_bstore(v, cr, co);
    }
  }
}

template <int NB>
int launch_nb(const OctM16P& p, int x16, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128 + 7);
  if (groups > 0x7fffffffLL) return -5;
  void (*const k[2][2])(OctM16P) = {{octant_rows_m16_kernel<NB, false, false>, octant_rows_m16_kernel<NB, false, true>},
                                    {octant_rows_m16_kernel<NB, true, false>, octant_rows_m16_kernel<NB, true, true>}};
  hipLaunchKernelGGL(k[mode == 3][x16 != 0], dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace

// mode: 2 bf16 / 3 fp16 (csn_capi.hip has checked it, and that the thread's rows16 flag is set)
int csn_launch_octant_down_bn_act_fwd_m16(const CsnOctantM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  CsnSparseConvM16Args g{};
  g.x = a.x; g.x16 = a.x16; g.ld_x = a.ld_x; g.n_in = a.n_fine; g.table = a.children; g.n_out = a.n_coarse; g.kv = 8;
  g.c_in = a.c_in; g.c_out = a.c_out; g.w = a.w; g.r = a.r; g.r16 = a.r16; g.ld_r = a.ld_r; g.y = a.y; g.y16 = a.y16; g.ld_y = a.ld_y;
  return csn_launch_sparse_conv_bn_act_fwd_m16(g, n, mode, st);
}

int csn_launch_octant_up_bn_act_fwd_m16(const CsnOctantM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  if (mode != 2 && mode != 3) return -1;
  OctM16P p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_coarse; p.parent = a.parent; p.order = a.order; p.seg = a.seg; p.b = a.w;
  p.c_in = a.c_in; p.c_out = a.c_out; p.c = a.y; p.ldc = a.ld_y; p.M = a.n_fine; p.K = a.c_in; p.J = a.c_out;
  p.gamma = n.gamma; p.beta = n.beta; p.rmean = n.running_mean; p.rvar = n.running_var; p.eps = n.eps;
  p.r = a.r; p.ldr = a.ld_r; p.relu = n.relu; p.r16 = a.r16; p.y16 = a.y16;
  return dispatch4(csn_octant_column_blocks(p.J, p.M), [&](auto nb) { return launch_nb<nb()>(p, a.x16, mode, st); });
}
