// Point fields: what MinkowskiNet puts around its sparse tensors (MinkowskiNet/lib/trainer_csn.py:236-260 the TensorField of a
// batch, :200-205 and :463-471 soutput.interpolate(field)).  Everything is POINT-MAJOR fp32 in every math mode (no product here).
//   voxel_mean    out[v] = (sum of feats[p] over the points of voxel v, in ascending point order) / count
//   interp_fwd    y[p]  = sum_{c in {0,1}^3} w_c(p) z[row(home(p) + c)],  w_c = prod_i (c_i ? t_i : 1 - t_i),  t = xyz - floor(xyz)
//                 formed in fp32; a corner with no voxel contributes nothing (it is never dereferenced)
//   interp_bwd    dz[v] = sum_c sum_{p : home(p) = v - c} w_c(p) dy[p]: OUTPUT-STATIONARY over the voxel rows.  Voxel v walks the eight
//                 corners in the fixed order c = cx + 2 cy + 4 cz = 0 .. 7 and, per present neighbour u = row(v - c), the points
//                 vox_pts[vox_ptr[u] .. vox_ptr[u + 1]) in order: no floating-point atomics, the same bits on every call.
// The corner rows come from the kernel-3 stride-1 map of the voxel set (table[27][n_voxels], -1 = no voxel):
//   row(v + c) = table[13 + cx + 3 cy + 9 cz][v],   row(v - c) = table[13 - cx - 3 cy - 9 cz][v].
// Thread layout (all three kernels): a row (a point, or a voxel) belongs to G consecutive lanes of one wave, G the power of two that
// holds the row's units (<= 64); a unit is 4 columns (16-byte accesses: VEC, every base 16-byte aligned and every pitch % 4 == 0; a
// width that is no multiple of 4 ends in a scalar tail) or one column.  A lane walks its units u = sub, sub + G, ...  The G lanes of
// a row read the same indices (one broadcast request); the eight neighbour rows and list bounds are all loaded before the first
// dependent read.  Every index read from memory is range-checked before it is used as one: an entry outside its array reads as
// "no voxel" / ends the list.
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int PF_BLOCK = 256;

struct PfGeom {
  int G, shift;            // lanes per row, log2
};

// t = x - floor(x) per axis and the eight corner weights, c = cx + 2 cy + 4 cz
CSN_DEVINL void pf_weights(const float* __restrict__ coords, long long p, float w[8]) {
  const f32x4 q = *reinterpret_cast<const f32x4*>(coords + p * 4);       // [b, x, y, z]: a 16-byte row
  const float tx = q.y - floorf(q.y), ty = q.z - floorf(q.z), tz = q.w - floorf(q.w);
  const float ax[2] = {1.f - tx, tx}, ay[2] = {1.f - ty, ty}, az[2] = {1.f - tz, tz};
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c] = (ax[c & 1] * ay[(c >> 1) & 1]) * az[c >> 2];
}

CSN_DEVINL float pf_weight(const float* __restrict__ coords, long long p, int c) {
  const f32x4 q = *reinterpret_cast<const f32x4*>(coords + p * 4);
  const float tx = q.y - floorf(q.y), ty = q.z - floorf(q.z), tz = q.w - floorf(q.w);
  return (((c & 1) ? tx : 1.f - tx) * ((c & 2) ? ty : 1.f - ty)) * ((c & 4) ? tz : 1.f - tz);
}

template <bool VEC>
__global__ __launch_bounds__(PF_BLOCK) void point_interp_fwd_kernel(const CsnPointFieldArgs a, const PfGeom g) {
  const long long p = ((long long)blockIdx.x * PF_BLOCK + threadIdx.x) >> g.shift;
  const int sub = threadIdx.x & (g.G - 1);
  if (p >= a.n_points) return;
  const int h = a.home[p];
  int row[8];
  float w[8];
  pf_weights(a.coords, p, w);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int r = -1;
    if ((unsigned)h < (unsigned)a.n_voxels) r = a.table[(long long)(13 + (c & 1) + 3 * ((c >> 1) & 1) + 9 * (c >> 2)) * a.n_voxels + h];
    row[c] = (unsigned)r < (unsigned)a.n_voxels ? r : -1;
  }
  float* __restrict__ y = a.y + p * a.ld_y;
  if constexpr (VEC) {
    const int c4 = a.C >> 2;
    for (int u = sub; u < c4; u += g.G) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (row[c] >= 0) acc += w[c] * *reinterpret_cast<const f32x4*>(a.z + (long long)row[c] * a.ld_z + u * 4);
      *reinterpret_cast<f32x4*>(y + u * 4) = acc;
    }
    for (int col = c4 * 4 + sub; col < a.C; col += g.G) {                // the scalar tail of a width % 4 != 0
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (row[c] >= 0) acc += w[c] * a.z[(long long)row[c] * a.ld_z + col];
      y[col] = acc;
    }
  } else {
    for (int col = sub; col < a.C; col += g.G) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (row[c] >= 0) acc += w[c] * a.z[(long long)row[c] * a.ld_z + col];
      y[col] = acc;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(PF_BLOCK) void point_interp_bwd_kernel(const CsnPointFieldArgs a, const PfGeom g) {
  const long long v = ((long long)blockIdx.x * PF_BLOCK + threadIdx.x) >> g.shift;
  const int sub = threadIdx.x & (g.G - 1);
  if (v >= a.n_voxels) return;
  int lo[8], hi[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int u = a.table[(long long)(13 - (c & 1) - 3 * ((c >> 1) & 1) - 9 * (c >> 2)) * a.n_voxels + v];
    int b = 0, e = 0;
    if ((unsigned)u < (unsigned)a.n_voxels) { b = a.vox_ptr[u]; e = a.vox_ptr[u + 1]; }
    lo[c] = max(b, 0);
    hi[c] = min(e, a.n_points);
  }
  float* __restrict__ dz = a.dz + v * a.ld_dz;
  const int c4 = VEC ? a.C >> 2 : 0;
  if constexpr (VEC) {
    for (int u = sub; u < c4; u += g.G) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c)
        for (int i = lo[c]; i < hi[c]; ++i) {
          const int p = a.vox_pts[i];
          if ((unsigned)p >= (unsigned)a.n_points) continue;
          acc += pf_weight(a.coords, p, c) * *reinterpret_cast<const f32x4*>(a.dy + (long long)p * a.ld_dy + u * 4);
        }
      *reinterpret_cast<f32x4*>(dz + u * 4) = acc;
    }
  }
  for (int col = c4 * 4 + sub; col < a.C; col += g.G) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      for (int i = lo[c]; i < hi[c]; ++i) {
        const int p = a.vox_pts[i];
        if ((unsigned)p >= (unsigned)a.n_points) continue;
        acc += pf_weight(a.coords, p, c) * a.dy[(long long)p * a.ld_dy + col];
      }
    dz[col] = acc;
  }
}

// C <= 64: one lane per column
__global__ __launch_bounds__(PF_BLOCK) void voxel_mean_kernel(const CsnPointFieldArgs a, const PfGeom g) {
  const long long v = ((long long)blockIdx.x * PF_BLOCK + threadIdx.x) >> g.shift;
  const int col = threadIdx.x & (g.G - 1);
  if (v >= a.n_voxels || col >= a.C) return;
  const int b = max(a.vox_ptr[v], 0), e = min(a.vox_ptr[v + 1], a.n_points);
  float acc = 0.f;
  int n = 0;
  for (int i = b; i < e; ++i) {
    const int p = a.vox_pts[i];
    if ((unsigned)p >= (unsigned)a.n_points) continue;
    acc += a.dy[(long long)p * a.ld_dy + col];
    ++n;
  }
  a.dz[v * a.ld_dz + col] = acc / (float)n;
}

PfGeom pf_geom(int units) {
  PfGeom g{1, 0};
  while (g.G < units && g.G < 64) { g.G <<= 1; ++g.shift; }
  return g;
}

unsigned pf_blocks(long long rows, const PfGeom& g) { return (unsigned)(((rows << g.shift) + PF_BLOCK - 1) / PF_BLOCK); }

bool pf_vec(const float* p, long long ld, const float* q, long long ldq) {
  return !((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) && !((ld | ldq) & 3);
}

}  // namespace

int csn_launch_point_interp_fwd(const CsnPointFieldArgs& a, hipStream_t st) {
  const bool vec = a.C >= 4 && pf_vec(a.z, a.ld_z, a.y, a.ld_y);
  const PfGeom g = pf_geom(vec ? (a.C + 3) >> 2 : a.C);
  if (vec) hipLaunchKernelGGL(point_interp_fwd_kernel<true>, dim3(pf_blocks(a.n_points, g)), dim3(PF_BLOCK), 0, st, a, g);
  else hipLaunchKernelGGL(point_interp_fwd_kernel<false>, dim3(pf_blocks(a.n_points, g)), dim3(PF_BLOCK), 0, st, a, g);
  return (int)hipGetLastError();
}

int csn_launch_point_interp_bwd(const CsnPointFieldArgs& a, hipStream_t st) {
  const bool vec = a.C >= 4 && pf_vec(a.dy, a.ld_dy, a.dz, a.ld_dz);
  const PfGeom g = pf_geom(vec ? (a.C + 3) >> 2 : a.C);
  if (vec) hipLaunchKernelGGL(point_interp_bwd_kernel<true>, dim3(pf_blocks(a.n_voxels, g)), dim3(PF_BLOCK), 0, st, a, g);
  else hipLaunchKernelGGL(point_interp_bwd_kernel<false>, dim3(pf_blocks(a.n_voxels, g)), dim3(PF_BLOCK), 0, st, a, g);
  return (int)hipGetLastError();
}

// feats ride in a.dy / a.ld_dy, the means in a.dz / a.ld_dz
int csn_launch_voxel_mean(const CsnPointFieldArgs& a, hipStream_t st) {
  const PfGeom g = pf_geom(a.C);
  hipLaunchKernelGGL(voxel_mean_kernel, dim3(pf_blocks(a.n_voxels, g)), dim3(PF_BLOCK), 0, st, a, g);
  return (int)hipGetLastError();
}
