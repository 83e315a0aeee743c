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
#include "sconv_a16_body.inc"

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
