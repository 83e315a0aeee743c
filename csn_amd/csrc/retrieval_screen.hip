// fp16 SCREEN of the ragged retrieval measure (retrieval.hip):
//     out[i][j] ~ mean_{n < n1_i} max_{m < n2_j} cos(f1[off1[i] + n], f2[off2[j] + m])      |out - exact| <= csn_retrieval_screen_eps(C)
// The exact measure ranks; this one only decides which candidates CANNOT be ranked (DESIGN.md "fp16 screen of the shape
// graph"): a candidate more than 2 eps below the K-th best screen score of its row is below K others in fp32.
//   prep   one wave per row: the row is normalised in fp32 (max(|x|, 1e-12) clamp), scaled by 2^7 and rounded ONCE to fp16 into an
//          image [row][Cp], Cp = the channel count zero-padded to a multiple of 32.  A unit row times 2^7 has every element that
//          can move a cosine by more than 2^-21 in the NORMAL fp16 range, so the bound holds whatever the matrix unit does with
//          fp16 subnormals.  The row is first scaled by a power of two taken from its largest element (exact), so the norm
//          neither overflows nor loses bits at any finite scale of the input.
//   sweep  a work-group owns 128 query points of one pair and keeps them in LDS for the whole sweep; the candidate's points
//          stream 64 at a time through a double-buffered LDS image (the next tile travels global -> registers while this one is
//          multiplied, registers -> the other buffer after it: one barrier per tile); v_mfma_f32_32x32x16_f16 with the
//          candidate point on the accumulator registers and the query point on the lanes, so the maximum over candidates is a
//          register reduction.  Both operands are "k contiguous": one 16-byte LDS read is one fragment, no transposed reads.
//          The work-group leaves one fixed-tree partial sum per (pair, tile); they are added in tile order in fp64.  No atomics.
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int SCREEN_SHIFT = 7;                        // image = unit row * 2^7; a product of two images carries 2^14
constexpr int SCREEN_MAX_IT = CSN_SCREEN_MAX_CP / 32;  // 16-byte pieces of a 64-row candidate tile per thread

__global__ __launch_bounds__(256) void csn_screen_prep_kernel(const float* __restrict__ f, short* __restrict__ img, long long rows,
                                                              int C, int Cp, float eps) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* __restrict__ p = f + row * C;
  float mx = 0.f;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, fabsf(p[c]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  // pw = 2^-e for mx = 1.f * 2^e (biased exponent clamped to the normal range: pw is a normal power of two, x * pw is exact)
  int e = (int)((__builtin_bit_cast(unsigned, mx) >> 23) & 0xffu);
  e = e < 1 ? 1 : (e > 253 ? 253 : e);
  const float pw = __builtin_bit_cast(float, (unsigned)(254 - e) << 23);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float y = p[c] * pw;
    s = __fadd_rn(s, __fmul_rn(y, y));                      // two roundings, never contracted: tests/retrieval_screen_ref.py restates the bits
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  // x / max(|x|, eps) = (x pw) / max(|x pw|, eps pw), times 2^7
  const float scale = (float)(1 << SCREEN_SHIFT) / fmaxf(sqrtf(s), eps * pw);
  short* __restrict__ q = img + row * Cp;
  for (int c = lane; c < Cp; c += 64) q[c] = c < C ? csn_mode::to16<true>(p[c] * pw * scale) : (short)0;
}

// part[pair * tiles + tile] = sum over the tile's query points n of max_m <img1[n], img2[m]> * 2^-14
__global__ __launch_bounds__(256) void csn_screen_sweep_kernel(const short* __restrict__ h1, const short* __restrict__ h2,
                                                               const int* __restrict__ off1, const int* __restrict__ off2,
                                                               float* __restrict__ part, int s2, int tiles, int Cp) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  const int pitch = Cp + 8;                                 // 16-byte reads of 16 rows cover the 64 banks once
  short* Qs = lds;                                          // [128 query points][pitch]
  short* Cs = lds + 128 * pitch;                            // [2][64 candidate points][pitch]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int pair = blockIdx.x / tiles, i = pair / s2, j = pair % s2;
  const int nq0 = (blockIdx.x % tiles) * 128;
  const int r1 = off1[i], n1 = off1[i + 1] - r1;
  const int r2 = off2[j], n2 = off2[j + 1] - r2;
  if (nq0 >= n1) return;                                    // past the query shape (uniform over the work-group)

  const int cpr = Cp >> 3;                                  // 16-byte pieces per image row; a tile's pieces are contiguous in memory
  const int nit = Cp >> 5;                                  // 64 * cpr / 256 pieces of a candidate tile per thread (Cp % 32 == 0)
  {
    const csn_rsrc_t Qr = csn_make_rsrc(h1 + ((long long)r1 + nq0) * Cp, (long long)min(128, n1 - nq0) * Cp * 2);
    for (int q = tid; q < 128 * cpr; q += 256) {            // rows past the shape fall outside the window -> zeros
      const int row = q / cpr, c8 = q - row * cpr;
      *reinterpret_cast<f32x4*>(&Qs[row * pitch + c8 * 8]) = csn_bload4(Qr, (unsigned)q * 16u);
    }
  }
  int prow[SCREEN_MAX_IT];                                  // LDS position of this thread's pieces of a candidate tile
#pragma unroll
  for (int it = 0; it < SCREEN_MAX_IT; ++it) {
    const int q = tid + 256 * it, row = q / cpr;
    prow[it] = row * pitch + (q - row * cpr) * 8;
  }
  f32x4 pre[SCREEN_MAX_IT];
  auto fetch = [&](int m0) {
    const csn_rsrc_t Cr = csn_make_rsrc(h2 + ((long long)r2 + m0) * Cp, (long long)min(64, n2 - m0) * Cp * 2);
#pragma unroll
    for (int it = 0; it < SCREEN_MAX_IT; ++it)
      if (it < nit) pre[it] = csn_bload4(Cr, (unsigned)(tid + 256 * it) * 16u);
  };
  auto stage = [&](short* buf) {
#pragma unroll
    for (int it = 0; it < SCREEN_MAX_IT; ++it)
      if (it < nit) *reinterpret_cast<f32x4*>(&buf[prow[it]]) = pre[it];
  };
  fetch(0);
  stage(Cs);
  __syncthreads();

  const short* __restrict__ qrow = Qs + (32 * wave + l31) * pitch + 8 * h;   // this wave's 32 query points
  float best = -INFINITY;
  int b = 0;
  for (int m0 = 0; m0 < n2; m0 += 64, b ^= 1) {
    const bool more = m0 + 64 < n2;
    if (more) fetch(m0 + 64);
    const short* __restrict__ c0 = Cs + b * 64 * pitch + l31 * pitch + 8 * h;
    const short* __restrict__ c1 = c0 + 32 * pitch;
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    // two 16-channel steps per trip (Cp % 32 == 0); the next trip's six fragments are read while this trip's four products run
    s16x8 fr[6], nx[6];
    auto frags = [&](s16x8* f, int k) {
      f[0] = *reinterpret_cast<const s16x8*>(qrow + k);
      f[1] = *reinterpret_cast<const s16x8*>(c0 + k);
      f[2] = *reinterpret_cast<const s16x8*>(c1 + k);
      f[3] = *reinterpret_cast<const s16x8*>(qrow + k + 16);
      f[4] = *reinterpret_cast<const s16x8*>(c0 + k + 16);
      f[5] = *reinterpret_cast<const s16x8*>(c1 + k + 16);
    };
    frags(fr, 0);
    for (int k = 0; k < Cp; k += 32) {
      frags(nx, k + 32 < Cp ? k + 32 : k);                  // (the last trip reads its own fragments again: in bounds, unused)
      acc[0] = csn_mode::mfma32<true>(fr[1], fr[0], acc[0]);
      acc[1] = csn_mode::mfma32<true>(fr[2], fr[0], acc[1]);
      acc[0] = csn_mode::mfma32<true>(fr[4], fr[3], acc[0]);
      acc[1] = csn_mode::mfma32<true>(fr[5], fr[3], acc[1]);
#pragma unroll
      for (int t = 0; t < 6; ++t) fr[t] = nx[t];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 32 * a + csn_acc_row(r, h);
        if (m < n2) best = fmaxf(best, acc[a][r]);          // rows past the candidate's points are never candidates
      }
    if (more) stage(Cs + (b ^ 1) * 64 * pitch);
    __syncthreads();                                        // this tile consumed by every wave, the next one in place
  }
  best = fmaxf(best, csn_xhalf(best)) * (1.f / (float)(1 << (2 * SCREEN_SHIFT)));     // exact: a power of two
  float* sum = reinterpret_cast<float*>(lds);               // (the loop ended on a barrier: nobody reads Qs any more)
  if (h == 0) sum[32 * wave + l31] = nq0 + 32 * wave + l31 < n1 ? best : 0.f;
  __syncthreads();
  for (int o = 64; o > 0; o >>= 1) {                        // fixed tree: bitwise reproducible
    if (tid < o) sum[tid] += sum[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = sum[0];
}

}  // namespace

int csn_screen_padded_channels(int C) { return (C + 31) / 32 * 32; }

int csn_launch_ragged_retrieval_screen_f16(const float* f1, const int* off1, int s1, long long N1, const float* f2, const int* off2,
                                           int s2, long long N2, int max_n1, int C, float* out, float* ws, hipStream_t st) {
  const int Cp = csn_screen_padded_channels(C);
  short* h1 = reinterpret_cast<short*>(ws);
  short* h2 = h1 + N1 * Cp;
  float* part = ws + (N1 + N2) * (Cp / 2);
  const int tiles = (max_n1 + 127) / 128;
  const long long blocks = (long long)tiles * s1 * s2;
  if (blocks > 0x7fffffffLL) return -1;                    // CSN_E_ARG: score fewer query shapes per call
  const int lds_bytes = 256 * (Cp + 8) * 2;
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(csn_screen_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       lds_bytes);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(csn_screen_prep_kernel, dim3((unsigned)((N1 + 3) / 4)), dim3(256), 0, st, f1, h1, N1, C, Cp, 1e-12f);
  hipLaunchKernelGGL(csn_screen_prep_kernel, dim3((unsigned)((N2 + 3) / 4)), dim3(256), 0, st, f2, h2, N2, C, Cp, 1e-12f);
  hipLaunchKernelGGL(csn_screen_sweep_kernel, dim3((unsigned)blocks), dim3(256), lds_bytes, st, h1, h2, off1, off2, part, s2, tiles, Cp);
  return csn_launch_ragged_mean_f32(part, off1, out, s1 * s2, s2, tiles, st);      // tile order, fp64: the exact measure's mean
}
