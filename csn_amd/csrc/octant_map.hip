// Octant maps: the partition of a fine coordinate set by its coarse set (csn_amd/minkowski_conv.py build_octant_map,
// csn_amd/minkowski_unet.py build_unet_pyramid) as integer kernels on the packed keys of kernel_map.hip:
//   key = b << 48 | (x + 2^15) << 32 | (y + 2^15) << 16 | (z + 2^15).
//   octant_partition   per fine row i: the key of [b, floor(xyz / 2ts) 2ts] (floor per field after unpacking, the batch field is not
//                      touched), ONE lower-bound search for it in the ascending coarse keys; parent[i] = its row or -1, octant[i] =
//                      ox + 2 oy + 4 oz with o = (xyz - floor(xyz / 2ts) 2ts) / ts, children[octant[i]][parent[i]] = i.  The entry
//                      point fills children with -1 before the launch.  Unique fine rows give every (octant, parent) slot at most
//                      one writer: no atomics on data.  status |= 8 where two neighbours of the coarse keys (or of the sorted fine
//                      keys, where the caller hands them in) are equal or descending | 16 where a parent is not in the coarse set.
//   octant_order       order = the rows sorted by (octant, row), seg = the segment bounds: a stable counting sort in three launches.
//                      (1) count: a tile of OO_TILE rows per work-group, one row per thread; per octant one wave ballot, its
//                      population count per wave into LDS, the waves' sum into counts[octant][tile].  (2) scan: ONE work-group
//                      walks the 8 x tiles counts octant by octant, OO_SCAN tiles per pass (wave prefix by __shfl_up, the waves'
//                      totals through LDS, a running carry over the passes and octants), turning every count into the tile's first
//                      position in order and the carry after octant k into seg[k + 1].  (3) scatter: the same ballots again; a row's
//                      rank inside its tile is the population count of its octant's ballot below its lane plus the counts of the
//                      waves before its own.  Every position is computed, none is drawn from a counter: the same integers on every
//                      call.  An entry outside [0, 8) is counted nowhere and written nowhere: status |= 32.
// Offsets into children and counts are 64-bit.  The status flags of a wave are or-ed across its lanes and leave it as one atomicOr,
// issued only by a wave that found something.  The search position is computed, never read; a row number read from coarse_rows that
// lies outside [0, n_coarse) reads as "no parent"; a position outside [0, n) is not written.
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int OM_BLOCK = 256;
constexpr int OM_FIELD = 16, OM_BIAS = 1 << (OM_FIELD - 1);
constexpr long long OM_MASK = (1ll << OM_FIELD) - 1;
constexpr int OO_TILE = CSN_OCTANT_ORDER_TILE, OO_SCAN = CSN_OCTANT_ORDER_SCAN, OO_WAVES = OO_TILE / 64;
static_assert(OO_TILE % 64 == 0 && OO_SCAN % 64 == 0, "whole waves");

// every lane must arrive (no early return before this)
CSN_DEVINL void om_flag(int f, int* __restrict__ status) {
  if (__ballot(f != 0) == 0ull) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) f |= __shfl_xor(f, d, 64);
  if ((threadIdx.x & 63) == 0) atomicOr(status, f);
}

CSN_DEVINL long long om_floor_to(long long v, long long s) {
  long long q = v / s;
  if (v % s < 0) --q;                                                   // s > 0: C++ truncates, the set is defined by floor
  return q * s;
}

__global__ __launch_bounds__(OM_BLOCK) void octant_partition_kernel(const CsnOctantMapArgs a) {
  const long long i = (long long)blockIdx.x * OM_BLOCK + threadIdx.x;
  int f = 0;
  if (i + 1 < a.n_coarse && a.coarse_keys[i] >= a.coarse_keys[i + 1]) f = 8;
  if (a.fine_sorted && i + 1 < a.n_fine && a.fine_sorted[i] >= a.fine_sorted[i + 1]) f = 8;
  if (i < a.n_fine) {
    const long long key = a.fine_keys[i];
    const long long batch = key & ~((1ll << (3 * OM_FIELD)) - 1);
    const long long x = ((key >> (2 * OM_FIELD)) & OM_MASK) - OM_BIAS, y = ((key >> OM_FIELD) & OM_MASK) - OM_BIAS, z = (key & OM_MASK) - OM_BIAS;
    const long long s = a.tensor_stride, s2 = 2 * s;
    const long long px = om_floor_to(x, s2), py = om_floor_to(y, s2), pz = om_floor_to(z, s2);
    const int oct = (int)((x - px) / s + 2 * ((y - py) / s) + 4 * ((z - pz) / s));       // every term's quotient is 0 or 1: [0, 8)
    int par = -1;
    if (px >= -OM_BIAS && py >= -OM_BIAS && pz >= -OM_BIAS) {            // (a floor never rises: the upper edge holds)
      const long long q = batch | ((px + OM_BIAS) << (2 * OM_FIELD)) | ((py + OM_BIAS) << OM_FIELD) | (pz + OM_BIAS);
      int pos = 0, hi = a.n_coarse;                                       // lower bound: the first position whose key is >= q
      while (pos < hi) {
        const int mid = pos + ((hi - pos) >> 1);
        if (a.coarse_keys[mid] < q) pos = mid + 1; else hi = mid;
      }
      if (pos < a.n_coarse && a.coarse_keys[pos] == q) {
        const int v = a.coarse_rows ? a.coarse_rows[pos] : pos;
        if ((unsigned)v < (unsigned)a.n_coarse) par = v;
      }
    }
    a.parent[i] = par;
    a.octant[i] = oct;
    if (par < 0) f |= 16;
    else a.children[(long long)oct * a.n_coarse + par] = (int)i;          // (64-bit offset)
  }
  om_flag(f, a.status);
}

// the ballots of a tile: cnt[w][o] = the rows of wave w in octant o; returns the rows of the caller's octant below its lane
CSN_DEVINL int oo_ballots(int k, int (*cnt)[8]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int rank = 0;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const unsigned long long m = __ballot(k == o);
    if (lane == o) cnt[w][o] = __popcll(m);
    if (k == o) rank = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  return rank;
}

__global__ __launch_bounds__(OO_TILE) void octant_count_kernel(const int* __restrict__ octant, int n, long long tiles,
                                                               int* __restrict__ counts, int* __restrict__ status) {
  __shared__ int cnt[OO_WAVES][8];
  const long long i = (long long)blockIdx.x * OO_TILE + threadIdx.x;
  int k = -1, f = 0;
  if (i < n) {
    k = octant[i];
    if ((unsigned)k >= 8u) { k = -1; f = 32; }
  }
  oo_ballots(k, cnt);
  if (threadIdx.x < 8) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < OO_WAVES; ++w) sum += cnt[w][threadIdx.x];
    counts[threadIdx.x * tiles + blockIdx.x] = sum;
  }
  om_flag(f, status);
}

__global__ __launch_bounds__(OO_SCAN) void octant_scan_kernel(int* __restrict__ counts, long long tiles, int* __restrict__ seg) {
  __shared__ int wave_sum[OO_SCAN / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;                                                          // the rows before this pass: the same in every thread
  if (threadIdx.x == 0) seg[0] = 0;
  for (int k = 0; k < 8; ++k) {
    for (long long base = 0; base < tiles; base += OO_SCAN) {
      const long long t = base + threadIdx.x;
      const int c = t < tiles ? counts[k * tiles + t] : 0;
      int incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
      }
      if (lane == 63) wave_sum[w] = incl;
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int j = 0; j < OO_SCAN / 64; ++j) {
        const int v = wave_sum[j];
        if (j < w) before += v;
        total += v;
      }
      if (t < tiles) counts[k * tiles + t] = carry + before + incl - c;   // the tile's first position in order
      carry += total;
      __syncthreads();                                                    // wave_sum is written again in the next pass
    }
    if (threadIdx.x == 0) seg[k + 1] = carry;
  }
}

__global__ __launch_bounds__(OO_TILE) void octant_scatter_kernel(const int* __restrict__ octant, int n, long long tiles,
                                                                 const int* __restrict__ first, int* __restrict__ order) {
  __shared__ int cnt[OO_WAVES][8];
  const long long i = (long long)blockIdx.x * OO_TILE + threadIdx.x;
  int k = -1;
  if (i < n) {
    k = octant[i];
    if ((unsigned)k >= 8u) k = -1;
  }
  const int rank = oo_ballots(k, cnt);
  if (k < 0) return;
  const int w = threadIdx.x >> 6;
  int before = 0;
#pragma unroll
  for (int j = 0; j < OO_WAVES; ++j)
    if (j < w) before += cnt[j][k];
  const long long pos = (long long)first[k * tiles + blockIdx.x] + before + rank;
  if (pos >= 0 && pos < n) order[pos] = (int)i;
}

unsigned om_blocks(long long n) { return (unsigned)((n + OM_BLOCK - 1) / OM_BLOCK); }

}  // namespace

// one thread per fine row; the neighbour checks ride in the same grid, so it covers max(n_fine, n_coarse - 1) threads
int csn_launch_octant_partition(const CsnOctantMapArgs& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.children, 0xFF, (size_t)8 * a.n_coarse * sizeof(int), st);       // every entry -1
  if (e != hipSuccess) return (int)e;
  const long long threads = a.n_fine > a.n_coarse - 1 ? a.n_fine : a.n_coarse - 1;
  hipLaunchKernelGGL(octant_partition_kernel, dim3(om_blocks(threads)), dim3(OM_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

long long csn_octant_order_tiles(int n) { return ((long long)n + OO_TILE - 1) / OO_TILE; }

int csn_launch_octant_order(const int* octant, int n, int* order, int* seg, int* counts, int* status, hipStream_t st) {
  const long long tiles = csn_octant_order_tiles(n);
  hipLaunchKernelGGL(octant_count_kernel, dim3((unsigned)tiles), dim3(OO_TILE), 0, st, octant, n, tiles, counts, status);
  hipLaunchKernelGGL(octant_scan_kernel, dim3(1), dim3(OO_SCAN), 0, st, counts, tiles, seg);
  hipLaunchKernelGGL(octant_scatter_kernel, dim3((unsigned)tiles), dim3(OO_TILE), 0, st, octant, n, tiles, (const int*)counts, order);
  return (int)hipGetLastError();
}
