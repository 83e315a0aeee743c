// Resident point collections (csn_amd/minkowski_points.py, include/csn_hip.h section 18): a category's points live on the device as
// one flat [N][3] fp32 array plus a CSR of shapes; a batch is normalised once and then augmented, voxel-scaled, keyed and collated
// by the kernels below.  Everything is float64 arithmetic on the fp32 inputs with EVERY operation rounded on its own: contraction is
// switched off for this file, so a product and the add behind it are never fused (the bit statement of section 18 depends on it;
// the division and the square root keep the fused steps of their own correctly rounded expansions).
//   normalize    one work-group per shape: c = (sum p) / n, r = the bounding-sphere radius or the bounding-box diagonal of p - c,
//                clamped to 2 eps_fp32; out = fp32((p - c) / r).  The sum is per-thread strided partials, then a fixed tree in LDS.
//   bounds       one work-group per batch item: min and max per axis of the item's points rotated about y (exact, order-free)
//   batch        grid (chunks of a shape, items): rotate, shift (clipped, scaled by the bounding-box diagonal of bounds), jitter,
//                scale; feats = fp32(q), coords = [item, fp32(q / voxel_size)], keys = the packed key of the floors, labels gathered
//   field_index  one thread per sorted point: home, the CSR heads and the unique keys of a PointField from its sorted keys
// No floating-point atomics anywhere: two calls give the same bits.  Status flags leave a wave as one atomicOr (an integer or of a
// caller-zeroed word), issued only by a wave that found something.  A shape index, a CSR offset, an output row or a voxel number
// outside its array is never used as an address: the item (or the point) is skipped and flagged.
#pragma clang fp contract(off)
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_FIELD = 16, PT_BIAS = 1 << (PT_FIELD - 1), PT_BATCH = 1 << 15;
constexpr int PT_F_BATCH = 1, PT_F_RANGE = 2, PT_F_FINITE = 16, PT_F_INDEX = 32;

// every lane of the wave must arrive (no early return of single lanes before this)
CSN_DEVINL void pt_flag(int f, int* __restrict__ status) {
  if (__ballot(f != 0) == 0ull) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) f |= __shfl_xor(f, d, 64);
  if ((threadIdx.x & 63) == 0) atomicOr(status, f);
}

// the rows [lo, hi) of shape s, or false where the CSR does not hold them inside [0, n_total]
CSN_DEVINL bool pt_shape(const long long* __restrict__ offsets, long long s, int n_shapes, long long n_total, long long& lo, long long& hi) {
  if (s < 0 || s >= n_shapes) return false;
  lo = offsets[s];
  hi = offsets[s + 1];
  return lo >= 0 && lo < hi && hi <= n_total;
}

// a fixed tree over the PT_BLOCK slots of `buf` (slot t belongs to thread t); every thread returns the result
template <typename Op> CSN_DEVINL double pt_tree(double v, double* buf, Op op) {
  const int t = threadIdx.x;
  __syncthreads();                                                  // the previous tree's readers are done with buf
  buf[t] = v;
  __syncthreads();
#pragma unroll
  for (int w = PT_BLOCK / 2; w > 0; w >>= 1) {
    if (t < w) buf[t] = op(buf[t], buf[t + w]);
    __syncthreads();
  }
  return buf[0];
}

struct PtAdd { CSN_DEVINL double operator()(double a, double b) const { return a + b; } };
struct PtMax { CSN_DEVINL double operator()(double a, double b) const { return b > a ? b : a; } };
struct PtMin { CSN_DEVINL double operator()(double a, double b) const { return b < a ? b : a; } };

__global__ __launch_bounds__(PT_BLOCK) void points_normalize_kernel(const CsnPointsArgs a) {
  __shared__ double buf[PT_BLOCK];
  long long lo = 0, hi = 0;
  const bool ok = pt_shape(a.offsets, blockIdx.x, a.n_shapes, a.n_total, lo, hi);      // uniform over the work-group
  pt_flag(ok ? 0 : PT_F_INDEX, a.status);
  if (!ok) return;
  const float* __restrict__ p = a.points;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
    sx += (double)p[i * 3];
    sy += (double)p[i * 3 + 1];
    sz += (double)p[i * 3 + 2];
  }
  const double n = (double)(hi - lo);
  const double cx = pt_tree(sx, buf, PtAdd()) / n, cy = pt_tree(sy, buf, PtAdd()) / n, cz = pt_tree(sz, buf, PtAdd()) / n;
  double r;
  if (a.method == 0) {                                               // sphere: sqrt of the largest squared distance
    double m = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
      const double dx = (double)p[i * 3] - cx, dy = (double)p[i * 3 + 1] - cy, dz = (double)p[i * 3 + 2] - cz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      m = d2 > m ? d2 : m;
    }
    r = sqrt(pt_tree(m, buf, PtMax()));
  } else {                                                           // box: the diagonal of the bounding box of p - c
    const double inf = __builtin_huge_val();
    double x0 = inf, y0 = inf, z0 = inf, x1 = -inf, y1 = -inf, z1 = -inf;
    for (long long i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
      const double dx = (double)p[i * 3] - cx, dy = (double)p[i * 3 + 1] - cy, dz = (double)p[i * 3 + 2] - cz;
      x0 = dx < x0 ? dx : x0; x1 = dx > x1 ? dx : x1;
      y0 = dy < y0 ? dy : y0; y1 = dy > y1 ? dy : y1;
      z0 = dz < z0 ? dz : z0; z1 = dz > z1 ? dz : z1;
    }
    const double ex = pt_tree(x1, buf, PtMax()) - pt_tree(x0, buf, PtMin());
    const double ey = pt_tree(y1, buf, PtMax()) - pt_tree(y0, buf, PtMin());
    const double ez = pt_tree(z1, buf, PtMax()) - pt_tree(z0, buf, PtMin());
    r = sqrt((ex * ex + ey * ey) + ez * ez);
  }
  const double floor_r = 2.0 * 1.1920928955078125e-07;              // 2 eps_fp32
  r = r > floor_r ? r : floor_r;                                     // (a NaN radius stays NaN: the outputs say so)
  float* __restrict__ out = a.out;
  for (long long i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {      // a thread rewrites only the points it reads here: in place is fine
    const double dx = (double)p[i * 3] - cx, dy = (double)p[i * 3 + 1] - cy, dz = (double)p[i * 3 + 2] - cz;
    out[i * 3] = (float)(dx / r);
    out[i * 3 + 1] = (float)(dy / r);
    out[i * 3 + 2] = (float)(dz / r);
  }
}

__global__ __launch_bounds__(PT_BLOCK) void points_bounds_kernel(const CsnPointsArgs a) {
  __shared__ double buf[PT_BLOCK];
  const int item = blockIdx.x;
  long long lo = 0, hi = 0;
  const bool ok = pt_shape(a.offsets, a.idx[item], a.n_shapes, a.n_total, lo, hi);     // uniform over the work-group
  pt_flag(ok ? 0 : PT_F_INDEX, a.status);
  double* __restrict__ out = a.bounds + (long long)item * 6;
  if (!ok) {
    if (threadIdx.x < 6) out[threadIdx.x] = 0.0;
    return;
  }
  const double c = a.params[(long long)item * CSN_POINTS_NPARAM], s = a.params[(long long)item * CSN_POINTS_NPARAM + 1];
  const double ns = -s;
  const float* __restrict__ p = a.points;
  const double inf = __builtin_huge_val();
  double x0 = inf, y0 = inf, z0 = inf, x1 = -inf, y1 = -inf, z1 = -inf;
  for (long long i = lo + threadIdx.x; i < hi; i += PT_BLOCK) {
    const double x = (double)p[i * 3], y = (double)p[i * 3 + 1], z = (double)p[i * 3 + 2];
    const double rx = c * x + s * z, rz = ns * x + c * z;
    x0 = rx < x0 ? rx : x0; x1 = rx > x1 ? rx : x1;
    y0 = y < y0 ? y : y0;   y1 = y > y1 ? y : y1;
    z0 = rz < z0 ? rz : z0; z1 = rz > z1 ? rz : z1;
  }
  x0 = pt_tree(x0, buf, PtMin()); y0 = pt_tree(y0, buf, PtMin()); z0 = pt_tree(z0, buf, PtMin());
  x1 = pt_tree(x1, buf, PtMax()); y1 = pt_tree(y1, buf, PtMax()); z1 = pt_tree(z1, buf, PtMax());
  if (threadIdx.x == 0) {
    out[0] = x0; out[1] = y0; out[2] = z0; out[3] = x1; out[4] = y1; out[5] = z1;
  }
}

CSN_DEVINL bool pt_finite(double v) { return __builtin_fabs(v) < __builtin_huge_val(); }     // false for NaN and +-inf
CSN_DEVINL double pt_clip(double v, double c) { return v < -c ? -c : (v > c ? c : v); }       // a NaN stays a NaN

__global__ __launch_bounds__(PT_BLOCK) void points_batch_kernel(const CsnPointsArgs a) {
  const int item = blockIdx.y;
  long long lo = 0, hi = 0;
  int f = 0;
  bool ok = pt_shape(a.offsets, a.idx[item], a.n_shapes, a.n_total, lo, hi);           // uniform over the work-group
  const long long row0 = a.out_offsets[item];
  if (ok && (row0 < 0 || row0 > a.n_out || hi - lo > a.n_out - row0)) ok = false;
  if (!ok) f |= PT_F_INDEX;
  const long long j = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (ok && j < hi - lo) {
    const double* __restrict__ pr = a.params + (long long)item * CSN_POINTS_NPARAM;
    const double* __restrict__ bb = a.bounds + (long long)item * 6;
    const double c = pr[0], s = pr[1], scale = pr[8];
    const double ns = -s;
    const double ex = bb[3] - bb[0], ey = bb[4] - bb[1], ez = bb[5] - bb[2];
    const double diag = sqrt((ex * ex + ey * ey) + ez * ez);
    const double sd = a.sigma * diag;
    bool fin = pt_finite(c) && pt_finite(s) && pt_finite(scale);
    const float* __restrict__ p = a.points + (lo + j) * 3;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double r[3] = {c * x + s * z, y, ns * x + c * z};
    float q32[3], v32[3];
    long long fl[3];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      fin = fin && pt_finite(pr[2 + k]) && pt_finite(pr[5 + k]);
      const double t = pt_clip(sd * pr[2 + k], a.clip);
      const double q = ((r[k] + t) + pr[5 + k]) * scale;
      const double v = q / a.voxel_size;
      fin = fin && pt_finite(q) && pt_finite(v);
      q32[k] = (float)q;
      v32[k] = (float)v;
      const float g = floorf(v32[k]);                                 // floor of the STORED coordinate, as PointField takes it
      const bool in = g >= (float)-PT_BIAS && g < (float)PT_BIAS;     // false for NaN
      in_range = in_range && in;
      fl[k] = in ? (long long)g : 0;
    }
    if (!fin) f |= PT_F_FINITE;
    else if (!in_range) f |= PT_F_RANGE;
    if (item >= PT_BATCH) f |= PT_F_BATCH;
    const long long row = row0 + j;
    *reinterpret_cast<f32x4*>(a.coords + row * 4) = f32x4{(float)item, v32[0], v32[1], v32[2]};
    a.feats[row * 3] = q32[0];
    a.feats[row * 3 + 1] = q32[1];
    a.feats[row * 3 + 2] = q32[2];
    a.keys[row] = (fin && in_range && item < PT_BATCH)
                      ? (((long long)item << (3 * PT_FIELD)) | ((fl[0] + PT_BIAS) << (2 * PT_FIELD)) | ((fl[1] + PT_BIAS) << PT_FIELD) | (fl[2] + PT_BIAS))
                      : -1ll;                                         // a flagged point's key: no valid key is negative
    if (a.labels) a.labels_out[row] = (long long)a.labels[lo + j];
  }
  pt_flag(f, a.status);
}

__global__ __launch_bounds__(PT_BLOCK) void field_index_kernel(const long long* __restrict__ skeys, const long long* __restrict__ order,
                                                               const long long* __restrict__ vid, int n_points, int n_voxels,
                                                               int* __restrict__ home, int* __restrict__ vox_ptr, int* __restrict__ vox_pts,
                                                               long long* __restrict__ uniq, int* __restrict__ status) {
  const long long j = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  int f = 0;
  if (j < n_points) {
    const long long o = order[j], v = vid[j];
    const bool o_ok = o >= 0 && o < n_points, v_ok = v >= 0 && v < n_voxels;
    if (!o_ok || !v_ok) f = PT_F_INDEX;
    vox_pts[j] = o_ok ? (int)o : -1;
    if (o_ok) home[o] = v_ok ? (int)v : -1;
    const long long key = skeys[j];
    if (v_ok && (j == 0 || skeys[j - 1] != key)) {                   // a run head
      vox_ptr[v] = (int)j;
      uniq[v] = key;
    }
    if (j == 0) vox_ptr[n_voxels] = n_points;
  }
  pt_flag(f, status);
}

unsigned pt_blocks(long long n) { return (unsigned)((n + PT_BLOCK - 1) / PT_BLOCK); }

}  // namespace

int csn_launch_points_normalize(const CsnPointsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(points_normalize_kernel, dim3(a.n_shapes), dim3(PT_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

int csn_launch_points_bounds(const CsnPointsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(points_bounds_kernel, dim3(a.n_items), dim3(PT_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

// grid.y = the item (at most 65535: checked by the entry point), grid.x = the chunks of the longest shape
int csn_launch_points_batch(const CsnPointsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(points_batch_kernel, dim3(pt_blocks(a.max_points), a.n_items), dim3(PT_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

int csn_launch_field_index(const long long* skeys, const long long* order, const long long* vid, int n_points, int n_voxels, int* home,
                           int* vox_ptr, int* vox_pts, long long* uniq_keys, int* status, hipStream_t st) {
  hipLaunchKernelGGL(field_index_kernel, dim3(pt_blocks(n_points)), dim3(PT_BLOCK), 0, st, skeys, order, vid, n_points, n_voxels, home,
                     vox_ptr, vox_pts, uniq_keys, status);
  return (int)hipGetLastError();
}
