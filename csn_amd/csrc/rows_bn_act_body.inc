// What the BatchNorm row kernels of rows_bn_act.hip (fp32 maps) and train_maps16.hip (y / r as bf16 rows) share, included into each
// file's unnamed namespace: the kernels' argument, the thread layout, the backward's two passes over a span of rows and the host's
// copy of the C ABI's arguments.  Y16: p.y holds bf16 rows (pitch in elements) — the backward reads its ReLU mask from 8-byte
// runs of them; everything else is the same text, so the same sums in the same order.
constexpr int MAXT = 3;

struct BnActP {
  const float* z[MAXT]; int ld_z[MAXT];
  const float* mean[MAXT]; const float* scale[MAXT]; const float* gamma[MAXT]; const float* beta[MAXT];   // mean / scale: [G][C]
  float* dz[MAXT]; int ld_dz[MAXT];
  int M;
  long long n_rows; int C;
  int eval, relu; float eps;
  const float* r; int ld_r;
  float* y; int ld_y;                          // forward: written; backward: read
  const float* dy; int ld_dy;
  float* dr; int ld_dr;
  const float* coef;                           // pass 2, training: [G][1 + M][C] mean g', mean g' xhat_m
  double* part;                                // pass 1: [part][1 + M][C]; a part is a chunk, or what a chunk and a group share
  const int* grp; int G;                       // GROUPED only: [G + 1] row offsets of the groups
  int n_parts;                                 // GROUPED only: chunks + G - 1, the bound of the part index
};

__device__ __forceinline__ float inv_std(const BnActP& p, int m, int c, bool eval) {
  return eval ? 1.f / sqrtf(p.scale[m][c] + p.eps) : p.scale[m][c];
}

// Thread layout of the three row kernels: 64 rows per work-group; a thread owns 4 consecutive channels (16-byte accesses on every
// map) of every RL-th row, RL = 256 / (C / 4) row lanes (32 at C = 32, 4 at C = 256; 240 of the 256 threads work at C = 96).  A
// thread's channels never change, so the terms' per-column constants sit in registers.
struct Lane { int rl, c, RL; bool on; };
__device__ __forceinline__ Lane lane_of(int C) {
  const int c4 = C >> 2, RL = 256 / c4, rl = (int)threadIdx.x / c4;
  return Lane{rl, ((int)threadIdx.x - rl * c4) * 4, RL, rl < RL};
}

// PASS 1: dr = g' and the span's fp64 column sums of g' and g' xhat_m, a thread's rows added in row order and left in LDS per row
// lane (store_part adds them).  PASS 2: dz_m.  The span: this thread's rows first, first + RL, ... < hi of the chunk at r0, the
// statistics at column offset so; the whole work-group calls.
template <int PASS, bool Y16 = false>
__device__ __forceinline__ void bwd_span(const BnActP& p, const Lane& t, long long r0, int first, int hi, int so, bool eval, double* sh) {
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[MAXT][4];
#pragma unroll
  for (int m = 0; m < MAXT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) s1[m][e] = 0.0;
  if (t.on) {
    float mu[MAXT][4], is[MAXT][4], gi[MAXT][4], cm[MAXT][4], c0[4];
    const bool use_coef = PASS == 2 && !eval;
    const float* coef = p.coef + (long long)so * (1 + p.M);
#pragma unroll
    for (int e = 0; e < 4; ++e) c0[e] = use_coef ? coef[t.c + e] : 0.f;
#pragma unroll
    for (int m = 0; m < MAXT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = m < p.M;
        mu[m][e] = in ? p.mean[m][so + t.c + e] : 0.f;
        is[m][e] = in ? inv_std(p, m, so + t.c + e, eval) : 0.f;
        gi[m][e] = in ? p.gamma[m][t.c + e] * is[m][e] : 0.f;
        cm[m][e] = (in && use_coef) ? coef[(1 + m) * p.C + t.c + e] : 0.f;
      }
#pragma unroll 2
    for (int rr = first; rr < hi; rr += t.RL) {
      const long long row = r0 + rr;
      f32x4 g = *reinterpret_cast<const f32x4*>(p.dy + row * p.ld_dy + t.c);
      if (p.relu) {
        f32x4 yv;
        if constexpr (Y16) yv = from16x4<false>(*reinterpret_cast<const s16x4*>(reinterpret_cast<const short*>(p.y) + row * p.ld_y + t.c));
        else yv = *reinterpret_cast<const f32x4*>(p.y + row * p.ld_y + t.c);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = yv[e] > 0.f ? g[e] : 0.f;
      }
      if constexpr (PASS == 1) {
        if (p.dr) *reinterpret_cast<f32x4*>(p.dr + row * p.ld_dr + t.c) = g;
#pragma unroll
        for (int e = 0; e < 4; ++e) s0[e] += (double)g[e];
      }
#pragma unroll
      for (int m = 0; m < MAXT; ++m) {
        if (m >= p.M) continue;
        if (PASS == 2 && !p.dz[m]) continue;
        if (PASS == 2 && eval) {
          f32x4 d;
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = g[e] * gi[m][e];
          *reinterpret_cast<f32x4*>(p.dz[m] + row * p.ld_dz[m] + t.c) = d;
          continue;
        }
        const f32x4 zv = *reinterpret_cast<const f32x4*>(p.z[m] + row * p.ld_z[m] + t.c);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (zv[e] - mu[m][e]) * is[m][e];
          if constexpr (PASS == 1) s1[m][e] += (double)g[e] * (double)xh;
          else d[e] = gi[m][e] * (g[e] - c0[e] - xh * cm[m][e]);
        }
        if constexpr (PASS == 2) *reinterpret_cast<f32x4*>(p.dz[m] + row * p.ld_dz[m] + t.c) = d;
      }
    }
  }
  if constexpr (PASS == 1) {
    if (t.on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sh[t.rl * p.C + t.c + e] = s0[e];
#pragma unroll
        for (int m = 0; m < MAXT; ++m)
          if (m < p.M) sh[((1 + m) * t.RL + t.rl) * p.C + t.c + e] = s1[m][e];
      }
    }
    __syncthreads();
  }
}

// the row lanes' sums of bwd_span<1>, added in lane order, as part `part_i`
__device__ __forceinline__ void store_part(const BnActP& p, const Lane& t, long long part_i, const double* sh) {
  for (int i = threadIdx.x; i < (1 + p.M) * p.C; i += 256) {
    const int q = i / p.C, col = i - q * p.C;
    double s = 0.0;
    for (int k = 0; k < t.RL; ++k) s += sh[(q * t.RL + k) * p.C + col];
    p.part[(part_i * (1 + p.M) + q) * p.C + col] = s;
  }
}

BnActP make_p(const CsnRowsBnActArgs& a, const int* group_rows, int n_groups) {
  BnActP p{};
  for (int m = 0; m < a.n_terms; ++m) {
    p.z[m] = a.z[m]; p.ld_z[m] = a.ld_z[m]; p.mean[m] = a.mean[m]; p.scale[m] = a.scale[m]; p.gamma[m] = a.gamma[m];
    p.beta[m] = a.beta[m]; p.dz[m] = a.dz[m]; p.ld_dz[m] = a.ld_dz[m];
  }
  p.M = a.n_terms; p.n_rows = a.n_rows; p.C = a.C; p.eval = !a.training && !group_rows; p.relu = a.relu; p.eps = a.eps;
  p.r = a.r; p.ld_r = a.ld_r; p.y = a.y; p.ld_y = a.ld_y; p.dy = a.dy; p.ld_dy = a.ld_dy; p.dr = a.dr; p.ld_dr = a.ld_dr;
  p.grp = group_rows; p.G = group_rows ? n_groups : 1;
  return p;
}
