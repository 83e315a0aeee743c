// Folded projections (csn_hip.h (1b)): the two product-free helpers of the fold.
//   csn_launch_tile_planes : x [item][rows][ldx] fp32  ->  bf16 tile planes, the layout csn_project_f32 writes with out_split = 2
//                            (wx_stream.hip OUT 2): per row and block of tb points 16 tiles of [hi 32 | lo 32], block pitch 1024,
//                            hi = bf16(x), lo = bf16(x - hi) (csn_mode::split4), the padding keys of a block's last tile zeros,
//                            tiles beyond a short last block not written.  Floor: 4 bytes read + 4 written per element.
//   csn_launch_transpose_f32: up to three small row-major matrices transposed in one launch (the fp32 GEMM takes its A operand
//                            k-contiguous only, and W_k^T W_q, W_v^T W_fc^T and W_fc^T dW_fv contract over A's rows).
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

using namespace csn_mode;

// one thread = one 16-byte unit of a tile: 8 keys, read as two 16-byte pieces, written as 16 bytes of hi and 16 of lo.
// Consecutive threads walk a row's units, so a wave reads 2 KB of the row in one piece and writes sixteen whole 128-byte lines.
__global__ __launch_bounds__(256) void csn_tile_planes_kernel(CsnTilePlanesArgs p) {
  const int cpb = (p.tb + 31) / 32;                                  // tiles per block
  const int nb = (p.n_points + p.tb - 1) / p.tb;
  const int uidx = blockIdx.x * 256 + threadIdx.x;                   // unit of the row
  if (uidx >= nb * cpb * 4) return;
  const int row = blockIdx.y, item = blockIdx.z;
  const int u = uidx & 3, tl = uidx >> 2, blk = tl / cpb, tile = tl - blk * cpb;
  const int t_blk = min(p.tb, p.n_points - blk * p.tb);              // points of this block (the last one may be short)
  if (t_blk - 32 * tile <= 0) return;                                // a tile beyond a short last block: not written
  const int k0 = 32 * tile + 8 * u;                                  // first key of the unit inside the block
  // (tb % 4 == 0 and n_points % 4 == 0: a 4-key piece is all in or all out)
  const float* src = p.x + (long long)item * p.x_item_stride + (long long)row * p.ldx + (long long)blk * p.tb + k0;
  f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
  if (k0 < t_blk) v0 = *reinterpret_cast<const f32x4*>(src);
  if (k0 + 4 < t_blk) v1 = *reinterpret_cast<const f32x4*>(src + 4);
  s16x4 h0, l0, h1, l1;
  split4<Bf16x3>(v0, h0, l0);
  split4<Bf16x3>(v1, h1, l1);
  // the row's descriptor is wave-uniform (row and item come from the block index); the unit's hi piece and, 64 bytes on, its lo
  const csn_rsrc_t Or = csn_make_rsrc(p.out + (long long)item * p.out_item_stride + (long long)row * p.ldo, (long long)p.ldo * 2);
  const unsigned off = (unsigned)(blk * 1024 + tile * 64 + 8 * u) * 2u;
  csn_bstore4(__builtin_bit_cast(f32x4, join8(h0, h1)), Or, off, 0u);
  csn_bstore4(__builtin_bit_cast(f32x4, join8(l0, l1)), Or, off, 64u);
}

// dst[c][r] = src[r][c], 32 x 32 tiles through LDS (pitch 33: both sides conflict-free); blockIdx.z = matrix
__global__ __launch_bounds__(256) void csn_transpose_kernel(CsnTransposeArgs p) {
  __shared__ float t[32][33];
  const float* src = p.src[blockIdx.z];
  float* dst = p.dst[blockIdx.z];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    if (r < p.rows && c < p.cols) t[ty + 8 * i][tx] = src[(long long)r * p.cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (r < p.rows && c < p.cols) dst[(long long)c * p.rows + r] = t[tx][ty + 8 * i];
  }
}

}  // namespace

int csn_launch_tile_planes(const CsnTilePlanesArgs& a, hipStream_t st) {
  if (a.n_items <= 0 || a.rows <= 0 || a.n_points <= 0) return 0;
  if (a.tb <= 0 || a.tb > 512 || (a.tb & 3) || (a.n_points & 3) || (a.ldx & 3) || (a.ldo & 7)) return -2;
  const int nb = (a.n_points + a.tb - 1) / a.tb;
  if ((long long)nb * 1024 > a.ldo || a.n_points > a.ldx) return -2;          // every block's 16 tiles lie inside the row
  if (a.rows > 65535 || a.n_items > 65535) return -2;
  const int units = nb * ((a.tb + 31) / 32) * 4;
  dim3 grid((unsigned)((units + 255) / 256), (unsigned)a.rows, (unsigned)a.n_items);
  hipLaunchKernelGGL(csn_tile_planes_kernel, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int csn_launch_transpose_f32(const CsnTransposeArgs& a, hipStream_t st) {
  if (a.n <= 0 || a.n > 3 || a.rows <= 0 || a.cols <= 0) return -2;
  dim3 grid((unsigned)((a.cols + 31) / 32), (unsigned)((a.rows + 31) / 32), (unsigned)a.n);
  hipLaunchKernelGGL(csn_transpose_kernel, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
}
