// The inference gather-GEMM of sparse_conv.hip on 16-bit maps (include/csn_hip.h section 24): the single-product forward
// (math modes 2 bf16 / 3 fp16 behind csn_set_thread_rows16) with the BatchNorm + residual + ReLU epilogue of section 19, where the
// gathered map x, the residual r and the output y may each be rows of the mode's 16-bit type instead of fp32.
//
//   sconv_maps16_kernel<NB, H16, A16>   the contraction of sconv_gemm16_bn_kernel<NB, H16> — the same offset list, the same
//                      (offset, 32-channel step) walk two steps ahead, W staged through LDS and rounded there, the same matrix
//                      instruction per (half step, column block) in the same order — so the accumulators are the same bits.
//                      A16: x holds 16-bit rows.  A lane's 16 values of a step are the runs k in [8 h, 8 h + 8) and
//                      [16 + 8 h, 16 + 8 h + 8): two 16-byte buffer loads at row * ld * 2 + (s % ks) * 64 + 16 h and + 32 that ARE
//                      the two A fragments (no conversion, no join: what to16x4 would have produced is what the map holds).
//                      !A16: x holds fp32 rows (the stem, conv1s1 reading out_init): the four loads and conversions of section 19.
//                      A -1 table entry and a row past the end give the lane CSN_OOB either way.
//   epilogue           v = fma(acc, s, t) (+ r), ReLU, exactly as store_tile_bn; r is read as fp32 or as 16-bit elements
//                      (converted exactly), y is stored as fp32 or as to16(v): ONE rounding to nearest even, overflow of an fp16
//                      store a plain conversion (inf).  The two types are wave-uniform runtime flags — the epilogue is not the
//                      hot loop, and flags keep the instances at NB x mode x A type = 16.  Each element of r is read and then
//                      written by the same lane, so r may be y.
// The launch rule is sparse_conv.hip's (csn_sconv_column_blocks): the same NB, hence the same summation order, as section 19.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

constexpr int MAX_KV = 125;

struct SconvM16P {
  const void* a; int lda; int n_src;   // A[n_src][lda]: the gathered map, fp32 or 16-bit rows (the kernel's A16), pitch in elements
  const int* table;                    // [KV][M]
  const float* b;                      // W[KV][c_in][c_out]
  int c_in, c_out;
  void* c; int ldc;                    // C[M][J], fp32 or 16-bit rows (y16)
  int M, K, J, KV;
  // the epilogue's arguments, read late (m16_args_late)
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps;
  const void* r; int ldr;              // residual [M][ldr], optional, fp32 or 16-bit rows (r16); may be c itself, same type and pitch
  int relu, r16, y16;
};
// As bn_args_late of sparse_conv.hip: the epilogue's arguments are read from the kernel-argument segment after the loop, so that
// they hold no scalar registers across it (the NB >= 2 instances have none to spare).
typedef const SconvM16P __attribute__((address_space(4)))* SconvM16LateP;
__device__ __forceinline__ SconvM16LateP m16_args_late() {
  SconvM16LateP k = (SconvM16LateP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// store_tile_bn with the residual and the output in either type (wave-uniform flags): the same wave-uniform row address + lane
// offset form, in bytes of the map's own element
template <bool H16>
__device__ __forceinline__ void store_tile_m16(const f32x16& acc, float s, float t, const void* r, int ldr, bool r16, bool relu, void* c,
                                               int ldc, bool y16, long long row_w, int cnt, int col, int h) {
  const int ysz = y16 ? 2 : 4, rsz = r16 ? 2 : 4;
  char* cw = static_cast<char*>(c) + row_w * ldc * ysz;
  const int lane = (4 * h * ldc + col) * ysz;
  const char* rw = r ? static_cast<const char*>(r) + row_w * ldr * rsz : nullptr;
  const int lane_r = (4 * h * ldr + col) * rsz;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    if (csn_acc_row(q, h) >= cnt) continue;
    float v = fmaf(acc[q], s, t);
    if (rw) {
      const char* ra = rw + csn_acc_row(q, 0) * ldr * rsz + lane_r;
      v += r16 ? from16<H16>(*reinterpret_cast<const short*>(ra)) : *reinterpret_cast<const float*>(ra);
    }
    v = relu ? fmaxf(0.f, v) : v;
    char* ca = cw + csn_acc_row(q, 0) * ldc * ysz + lane;
    if (y16) *reinterpret_cast<short*>(ca) = to16<H16>(v);
    else *reinterpret_cast<float*>(ca) = v;
  }
}

template <int NB, bool H16, bool A16>
__global__ __launch_bounds__(256) void sconv_maps16_kernel(const SconvM16P p) {
  constexpr int MODE = H16 ? 3 : 2;
  __shared__ __attribute__((aligned(16))) short Bs[NB * 32 * BS16_PITCH];
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
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * (A16 ? 2LL : 4LL));
  const unsigned a_in = (unsigned)(A16 ? 16 * h : 32 * h);            // byte offset of the lane's channels inside a 32-channel step
  const int ks = p.K >> 5;                                            // channel steps per offset

  // the offsets at which some row of the tile has a neighbour, in ascending order
  for (int k = tid; k < p.KV; k += 256) s_flag[k] = 0;
  __syncthreads();
  for (int k = 0; k < p.KV; ++k) {
    const int r = row_ok ? p.table[(long long)k * p.M + row_l] : -1;
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

  f32x16 acc[NB] = {};
  // step s = (offset s / ks of the list, channels 32 (s % ks) ..): the lane's source row of a step, two steps ahead of its use
  auto row_of = [&](int s) -> int {
    if (s >= S || !row_ok) return -1;
    return p.table[(long long)s_act[s / ks] * p.M + row_l];
  };
  constexpr int NA = A16 ? 2 : 4;                                     // 16-byte reads of A per lane and step
  f32x4 an[NA], bn[NB];
  auto load_a = [&](int s, int src) {
    if constexpr (A16) {
      const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 2u + a_in + (unsigned)((s % ks) * 64);
      an[0] = csn_bload4(ar, off);
      an[1] = csn_bload4(ar, off + 32u);
    } else {
      const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 4u + a_in + (unsigned)((s % ks) * 128);
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, off + (unsigned)(a_kofs<MODE>(g) * 4));
    }
  };
  auto load_w = [&](int s) {
    load_b<NB, true>(bn, p.b + (long long)s_act[s / ks] * p.c_in * p.c_out, p.c_out, (s % ks) * 32, j0, p.J, tid);
  };

  int r1 = row_of(0);
  if (S > 0) { load_a(0, r1); load_w(0); }
  r1 = row_of(1);
  int r2 = row_of(2);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, true, MODE>(Bs, bn, tid);
    f32x4 af[NA];
#pragma unroll
    for (int g = 0; g < NA; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) { load_a(s + 1, r1); load_w(s + 1); }
    r1 = r2;
    r2 = row_of(s + 3);
    if constexpr (A16) mma_step_a16<NB, H16>(acc, af, Bs, li, h);
    else mma_step<NB, MODE>(acc, af, Bs, li, h);
  }

  const long long row_w = row_g + wave * 32;                          // first row of the wave's tile
  const int cnt = (int)(p.M - row_w < 32 ? (p.M - row_w < 0 ? 0 : p.M - row_w) : 32);
  const auto* q = m16_args_late();
  const bool r16 = q->r16 != 0, y16 = q->y16 != 0;                     // wave-uniform
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = j0 + nb * 32 + li;
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    const float sc = q->gamma[col] / sqrtf(q->rvar[col] + q->eps);
    const float sh = q->beta[col] - q->rmean[col] * sc;
    const bool relu = q->relu != 0;
    store_tile_m16<H16>(acc[nb], sc, sh, q->r, q->ldr, r16, relu, p.c, p.ldc, y16, row_w, cnt, col, h);
  }
}

template <int NB>
int launch_nb(const SconvM16P& p, int x16, int mode, hipStream_t st) {
  const long long groups = (long long)((p.J + NB * 32 - 1) / (NB * 32)) * (((long long)p.M + 127) / 128);
  if (groups > 0x7fffffffLL) return -5;
  void (*const k[2][2])(SconvM16P) = {{sconv_maps16_kernel<NB, false, false>, sconv_maps16_kernel<NB, false, true>},
                                      {sconv_maps16_kernel<NB, true, false>, sconv_maps16_kernel<NB, true, true>}};
  hipLaunchKernelGGL(k[mode == 3][x16 != 0], dim3((unsigned)groups), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace

// mode: 2 bf16 / 3 fp16 (csn_capi.hip has checked it, and that the thread's rows16 flag is set)
int csn_launch_sparse_conv_bn_act_fwd_m16(const CsnSparseConvM16Args& a, const CsnSconvBnArgs& n, int mode, hipStream_t st) {
  if (mode != 2 && mode != 3) return -1;
  SconvM16P p{};
  p.a = a.x; p.lda = a.ld_x; p.n_src = a.n_in; p.table = a.table; p.b = a.w; p.c_in = a.c_in; p.c_out = a.c_out;
  p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = a.c_in; p.J = a.c_out; p.KV = a.kv;
  p.gamma = n.gamma; p.beta = n.beta; p.rmean = n.running_mean; p.rvar = n.running_var; p.eps = n.eps;
  p.r = a.r; p.ldr = a.ld_r; p.relu = n.relu; p.r16 = a.r16; p.y16 = a.y16;
  return dispatch4(csn_sconv_column_blocks(p.J, p.M), [&](auto nb) { return launch_nb<nb()>(p, a.x16, mode, st); });
}
