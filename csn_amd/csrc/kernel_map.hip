// Kernel maps: the coordinate manager of the sparse convolution (csn_amd/minkowski_conv.py build_kernel_map, csn_amd/minkowski_hrnet.py
// build_pyramid) as three integer kernels.  A coordinate [b, x, y, z] is one int64 key
//   key = b << 48 | (x + 2^15) << 32 | (y + 2^15) << 16 | (z + 2^15),   b in [0, 2^15), x, y, z in [-2^15, 2^15),
// whose order is the lexicographic order of (b, x, y, z): a coordinate set is its ascending key array, a lookup is a lower-bound
// search in it.  No hash table, no atomics on data: the tables are the integers the torch composition of sort and searchsorted
// gives, on every call.
//   coord_keys   keys[i] = key(coords[i]); status |= 1 (batch index out of range) | 2 (x, y or z out of range) | 4 (x, y or z no
//                multiple of the tensor stride)
//   coord_down   every field of a key floored to a multiple of the coarser tensor stride (floor, not truncation: -1 -> -2 at 2)
//   kernel_map   table[kidx][j] = row of "query j + step o(kidx)" in the set, or -1; kidx = (ox + r) + k (oy + r) + k^2 (oz + r).
//                The offset is added PER FIELD after unpacking: a field that leaves [0, 2^16) (biased) gives -1 and never carries
//                into its neighbour; the batch field is not touched.  status |= 8 where two neighbours of the set are equal or
//                descending.
// Thread layout: one thread per row.  In kernel_map a thread is a query row and loops over the k^2 pairs (ox, oy); the k offsets
// that share a pair are k keys |step| apart in the lowest field, so they take ONE lower-bound search (whose first levels are the
// same addresses in every lane) and a forward walk over the neighbouring entries: in a set whose z are multiples of the step the
// walk passes at most the k keys it looks for, in any ascending array it still ends at the right entry or at the array's end.
// Lane j stores table[kidx][j]: every store instruction of a wave is one contiguous piece.  Offsets into the table are 64-bit
// (KV n_query can exceed 2^31).  The status flags of a wave are or-ed across its lanes and leave it as one atomicOr, issued only by a
// wave that found something.  The search position is computed, never read; a row number read from set_rows that lies outside
// [0, n_set) reads as "no voxel".
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int KM_BLOCK = 256;
constexpr int KM_FIELD = 16, KM_BIAS = 1 << (KM_FIELD - 1), KM_BATCH = 1 << 15;
constexpr long long KM_MASK = (1ll << KM_FIELD) - 1;

CSN_DEVINL long long km_shl(long long v, int s) { return (long long)((unsigned long long)v << s); }

// what ((b << 48) | ((x + 2^15) << 32) | ((y + 2^15) << 16) | (z + 2^15)) is in 64-bit two's complement, in range or not
CSN_DEVINL long long km_pack(long long b, long long x, long long y, long long z) {
  return km_shl(b, 3 * KM_FIELD) | km_shl(x + KM_BIAS, 2 * KM_FIELD) | km_shl(y + KM_BIAS, KM_FIELD) | (z + KM_BIAS);
}

// every lane must arrive (no early return before this)
CSN_DEVINL void km_flag(int f, int* __restrict__ status) {
  if (__ballot(f != 0) == 0ull) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) f |= __shfl_xor(f, d, 64);
  if ((threadIdx.x & 63) == 0) atomicOr(status, f);
}

__global__ __launch_bounds__(KM_BLOCK) void coord_keys_kernel(const long long* __restrict__ coords, int n, long long ts,
                                                              long long* __restrict__ keys, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * KM_BLOCK + threadIdx.x;
  int f = 0;
  if (i < n) {
    const long long b = coords[i * 4], x = coords[i * 4 + 1], y = coords[i * 4 + 2], z = coords[i * 4 + 3];
    if (b < 0 || b >= KM_BATCH) f |= 1;
    if (x < -KM_BIAS || x >= KM_BIAS || y < -KM_BIAS || y >= KM_BIAS || z < -KM_BIAS || z >= KM_BIAS) f |= 2;
    if (x % ts != 0 || y % ts != 0 || z % ts != 0) f |= 4;              // a zero remainder is zero under floor and truncation alike
    keys[i] = km_pack(b, x, y, z);
  }
  km_flag(f, status);
}

CSN_DEVINL long long km_floor_to(long long v, long long s) {
  long long q = v / s;
  if (v % s < 0) --q;                                                   // s > 0: C++ truncates, the set is defined by floor
  return q * s;
}

__global__ __launch_bounds__(KM_BLOCK) void coord_down_kernel(const long long* __restrict__ keys, int n, long long ts,
                                                              long long* __restrict__ down) {
  const long long i = (long long)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const long long key = keys[i];
  const long long x = ((key >> (2 * KM_FIELD)) & KM_MASK) - KM_BIAS, y = ((key >> KM_FIELD) & KM_MASK) - KM_BIAS, z = (key & KM_MASK) - KM_BIAS;
  down[i] = km_pack(key >> (3 * KM_FIELD), km_floor_to(x, ts), km_floor_to(y, ts), km_floor_to(z, ts));
}

__global__ __launch_bounds__(KM_BLOCK) void kernel_map_kernel(const CsnKernelMapArgs a) {
  const long long j = (long long)blockIdx.x * KM_BLOCK + threadIdx.x;
  int f = 0;
  if (j + 1 < a.n_set && a.set_keys[j] >= a.set_keys[j + 1]) f = 8;
  if (j < a.n_query) {
    const long long key = a.query_keys[j];
    const long long batch = key & ~((1ll << (3 * KM_FIELD)) - 1);
    const int fx = (int)((key >> (2 * KM_FIELD)) & KM_MASK), fy = (int)((key >> KM_FIELD) & KM_MASK), fz = (int)(key & KM_MASK);
    const int k = a.kernel_size, r = k >> 1;
    const long long s = a.step < 0 ? -(long long)a.step : a.step;
    const long long plane = (long long)k * k * a.n_query;                 // table entries between two oz
    for (int oy = -r; oy <= r; ++oy) {
      const long long ny = fy + (long long)a.step * oy;
      for (int ox = -r; ox <= r; ++ox) {
        const long long nx = fx + (long long)a.step * ox;
        const bool ok = (unsigned long long)nx <= (unsigned long long)KM_MASK && (unsigned long long)ny <= (unsigned long long)KM_MASK;
        const long long run = batch | (nx << (2 * KM_FIELD)) | (ny << KM_FIELD);
        int* __restrict__ out = a.table + ((long long)((ox + r) + k * (oy + r)) * a.n_query + j);       // the entry of oz = -r
        // the k offsets that share (ox, oy) are k keys |step| apart in the lowest field: one lower-bound search for the lowest of
        // them, then a forward walk.  i counts them in ascending key order: z_i = z + |step| (i - r), oz = +-(i - r) by step's sign
        int pos = 0;
        if (ok) {
          const long long z0 = fz - s * r;
          const long long q = run | (z0 < 0 ? 0 : z0);
          int hi = a.n_set;                                               // lower bound: the first position whose key is >= q
          while (pos < hi) {
            const int mid = pos + ((hi - pos) >> 1);
            if (a.set_keys[mid] < q) pos = mid + 1; else hi = mid;
          }
        }
        for (int i = 0; i < k; ++i) {
          const long long nz = fz + s * (i - r);
          int row = -1;
          if (ok && (unsigned long long)nz <= (unsigned long long)KM_MASK) {
            const long long q = run | nz;
            while (pos < a.n_set && a.set_keys[pos] < q) ++pos;           // a valid set holds at most the k keys of the run here
            if (pos < a.n_set && a.set_keys[pos] == q) {
              const int v = a.set_rows ? a.set_rows[pos] : pos;
              if ((unsigned)v < (unsigned)a.n_set) row = v;
            }
          }
          const int oz = a.step > 0 ? i - r : r - i;
          out[(oz + r) * plane] = row;                                    // (64-bit offset)
        }
      }
    }
  }
  km_flag(f, a.status);
}

unsigned km_blocks(long long n) { return (unsigned)((n + KM_BLOCK - 1) / KM_BLOCK); }

}  // namespace

int csn_launch_coord_keys(const long long* coords, int n, int tensor_stride, long long* keys, int* status, hipStream_t st) {
  hipLaunchKernelGGL(coord_keys_kernel, dim3(km_blocks(n)), dim3(KM_BLOCK), 0, st, coords, n, (long long)tensor_stride, keys, status);
  return (int)hipGetLastError();
}

int csn_launch_coord_down(const long long* keys, int n, int out_tensor_stride, long long* down_keys, hipStream_t st) {
  hipLaunchKernelGGL(coord_down_kernel, dim3(km_blocks(n)), dim3(KM_BLOCK), 0, st, keys, n, (long long)out_tensor_stride, down_keys);
  return (int)hipGetLastError();
}

// one thread per query row; the set's neighbour check rides in the same grid, so it covers max(n_query, n_set - 1) threads
int csn_launch_kernel_map(const CsnKernelMapArgs& a, hipStream_t st) {
  const long long threads = a.n_query > a.n_set - 1 ? a.n_query : a.n_set - 1;
  hipLaunchKernelGGL(kernel_map_kernel, dim3(km_blocks(threads)), dim3(KM_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}
