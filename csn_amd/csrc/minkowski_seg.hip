// Everything between the MinkowskiNet head's logits and optimizer.step() / the reported metrics, on point-major ragged rows
// (MinkowskiNet/lib/trainer_csn.py:188-224 and :400-500, lib/utils.py:64-176):
//   forward   one pass over logits [N][ld] (n_classes <= ld): per row lse = log sum_c exp(z_c) and
//             pred = 1 + argmax_{1 <= c < n_classes} z_c (first maximum: torch.max(output[:, 1:], 1)[1] + 1, trainer_csn.py:466);
//             the sums of nn.CrossEntropyLoss(ignore_index) (:406, :471) and precision_at_one_partnet (utils.py:64-75);
//             per (segment, class) the three counts calculate_iou (utils.py:78-110) derives its intersections and unions from
//   backward  dz[n][c] = counted ? (exp(z_c - lse) - [c == label]) g / n_counted : 0; the label's own entry is formed as
//             expm1(-nll) from the row loss the forward kept (exp(z_label - lse) - 1 cancels for a confident row)
// Row classes (ignore = the ignore label):
//   counted   label != ignore and 0 <= label < n_classes: enters the loss, n_counted, n_correct and the counts
//   ignored   label == ignore: enters no loss sum; its prediction DOES enter pr (calculate_iou zeroes only ground == 0), and its
//             label enters gt when ignore < n_classes (ground == i is taken as it stands there)
//   bad       any other label (torch raises for it): enters n_bad and nothing else
// A row is 4 n_classes contiguous bytes, so a lane per row would read 64 strided rows: each wave stages its 64 rows through LDS
// at an odd pitch instead — the rows of a chunk are one contiguous run when ld <= 59 (16-byte loads where the base allows it) —
// and then reads its own row conflict-free.  Float sums leave as per-work-group fp64 partials added in a fixed order by a
// finishing kernel (bitwise reproducible); counts go through an LDS histogram per work-group and integer atomics (exact,
// order-independent).
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int SEG_ROWS = 64;              // rows per wave chunk
constexpr int SEG_WAVES = 4;
constexpr int SEG_BLOCK = SEG_ROWS * SEG_WAVES;
constexpr int SEG_COLS = 59;              // columns staged at once (odd: the pitch of a full chunk; 4 tiles + histogram < 64 KB of LDS)
constexpr int SEG_HIST_CLASSES = 256;     // widest class count of the LDS histogram
constexpr int SEG_HIST_SEGMENTS = 4;      // a work-group spanning more segments counts straight into global memory

// Running state of a row over its column chunks.  rest = sum_c exp(z_c - m) WITHOUT the maximum's own term (= 1): the row's
// loss is log1p(rest) + (m - z_label), two non-negative terms each good to a few ulp, where lse - z_label cancels (a confident
// row has lse - z_label ~ 1e-3 at |lse| ~ 4: one ulp of lse is 1e-4 of that loss).
struct SegRow {
  float m = -INFINITY, rest = 0.f, zl = 0.f, best = -INFINITY;
  int arg = 1;
};

// columns [c0, c0 + cc) of the lane's row, at t[0 .. cc)
CSN_DEVINL void seg_consume(SegRow& s, const float* t, int c0, int cc, long long lab) {
  for (int j = 0; j < cc; ++j) {
    const float v = t[j];
    const int c = c0 + j;
    if (v > s.m) {
      s.rest = (s.rest + 1.f) * expf(s.m - v);         // (the old maximum becomes one of the rest; the first class: (0 + 1) * 0)
      s.m = v;
    } else {
      s.rest += v == s.m ? 1.f : expf(v - s.m);        // (v == m: a tie, or a logit of -inf while the maximum still is)
    }
    if (c >= 1 && v > s.best) { s.best = v; s.arg = c; }   // strictly greater: the first maximum
    if (c == lab) s.zl = v;
  }
}

// the rows [0, rows) x columns [0, ld) of a chunk are one contiguous run of rows * ld floats: lane l takes the floats
// W (l + 64 k) .. + W - 1 and files each under (row, column) at the odd pitch
template <int W>
CSN_DEVINL void seg_stage_flat(csn_rsrc_t src, float* tile, int pitch, int rows, int ld, int lane) {
  const int total = rows * ld;
  int f = lane * W, r = f / ld, c = f - r * ld;
  const int step = 64 * W, dr = step / ld, dc = step - dr * ld;
  for (; f < total; f += step) {
    float v[W];
    if constexpr (W == 4) {
      if (f + 3 < total) {
        const f32x4 q = csn_bload4(src, (unsigned)f * 4u);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f + e < total ? csn_bload(src, (unsigned)(f + e) * 4u) : 0.f;
      }
    } else {
      v[0] = csn_bload(src, (unsigned)f * 4u);
    }
    int rr = r, cc = c;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      if (f + e < total) tile[rr * pitch + cc] = v[e];
      if (++cc == ld) { cc = 0; ++rr; }
    }
    r += dr; c += dc;
    if (c >= ld) { c -= ld; ++r; }
  }
}

// columns [c0, c0 + cc) of the rows [0, rows): lane l takes the elements l + 64 k of the rows x cc block
CSN_DEVINL void seg_stage_cols(csn_rsrc_t src, float* tile, int pitch, int rows, int ld, int c0, int cc, int lane) {
  const int total = rows * cc;
  int r = lane / cc, c = lane - r * cc;
  const int dr = 64 / cc, dc = 64 - dr * cc;
  for (int f = lane; f < total; f += 64) {
    tile[r * pitch + c] = csn_bload(src, (unsigned)(r * ld + c0 + c) * 4u);
    r += dr; c += dc;
    if (c >= cc) { c -= cc; ++r; }
  }
}

// the segment of a row: the s with offsets[s] <= row < offsets[s + 1]
CSN_DEVINL int seg_of_row(const int* __restrict__ offsets, int n_segments, int row) {
  int lo = 0, hi = n_segments;            // offsets[lo] <= row < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SEG_BLOCK) void csn_ragged_seg_fwd_kernel(CsnRaggedSegArgs p) {
  extern __shared__ float seg_tiles[];                          // SEG_WAVES tiles of SEG_ROWS x pitch
  __shared__ int hist[SEG_HIST_CLASSES * 3];
  __shared__ double red[4][SEG_WAVES];
  __shared__ int span[2];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = blockIdx.x * SEG_BLOCK + wave * SEG_ROWS;    // (n_rows < 2^31 - SEG_BLOCK: checked on the host)
  const int rows = min(SEG_ROWS, p.n_rows - row0);              // <= 0: the wave has no rows
  const int row = row0 + lane;
  const bool on = lane < rows;
  float* tile = seg_tiles + wave * (SEG_ROWS * p.pitch);

  long long lab = 0;
  SegRow s;
  if (rows > 0) {
    if (on) lab = p.labels[row];
    const csn_rsrc_t src = csn_make_rsrc(p.logits + (long long)row0 * p.ld, ((long long)(rows - 1) * p.ld + p.n_classes) * 4);
    if (p.ld <= SEG_COLS) {
      // (the run ends with the last row's classes: the pitch columns behind them belong to nobody)
      const csn_rsrc_t flat = csn_make_rsrc(p.logits + (long long)row0 * p.ld, (long long)rows * p.ld * 4);
      const int total_rows = rows == p.n_rows - row0 && p.ld > p.n_classes ? rows - 1 : rows;      // the last row of all: below
      if (p.vec) seg_stage_flat<4>(flat, tile, p.pitch, total_rows, p.ld, lane);
      else seg_stage_flat<1>(flat, tile, p.pitch, total_rows, p.ld, lane);
      if (total_rows < rows && lane < p.n_classes)              // its padding columns may lie past the allocation
        tile[total_rows * p.pitch + lane] = csn_bload(src, (unsigned)(total_rows * p.ld + lane) * 4u);
      __builtin_amdgcn_wave_barrier();
      if (on) seg_consume(s, tile + lane * p.pitch, 0, p.n_classes, lab);
    } else {
      for (int c0 = 0; c0 < p.n_classes; c0 += SEG_COLS) {
        const int cc = min(SEG_COLS, p.n_classes - c0);
        seg_stage_cols(src, tile, p.pitch, rows, p.ld, c0, cc, lane);
        __builtin_amdgcn_wave_barrier();
        if (on) seg_consume(s, tile + lane * p.pitch, c0, cc, lab);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }

  // per-row results
  const bool valid = on && lab >= 0 && lab < p.n_classes;
  const bool ignored = on && lab == p.ignore_label;
  const bool counted = valid && !ignored;
  const bool bad = on && !valid && !ignored;
  const float lrest = log1pf(s.rest);
  const float lse = s.m + lrest;
  if (on) {
    p.lse[row] = lse;
    p.nll[row] = counted ? lrest + (s.m - s.zl) : 0.f;
    p.pred[row] = s.arg;
  }
  double v_loss = counted ? (double)lrest + (double)(s.m - s.zl) : 0.0;
  double v_cnt = counted ? 1.0 : 0.0;
  double v_hit = counted && (s.arg == lab || lab == 0) ? 1.0 : 0.0;
  double v_bad = bad ? 1.0 : 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v_loss += __shfl_xor(v_loss, off, 64);
    v_cnt += __shfl_xor(v_cnt, off, 64);
    v_hit += __shfl_xor(v_hit, off, 64);
    v_bad += __shfl_xor(v_bad, off, 64);
  }
  if (lane == 0) { red[0][wave] = v_loss; red[1][wave] = v_cnt; red[2][wave] = v_hit; red[3][wave] = v_bad; }

  // counts: gt[label], pr[p'], inter[label] when they agree, p' = label == 0 ? 0 : pred.  A bad row enters none of them.
  const int gt_c = valid ? (int)lab : -1;
  const int pr_c = bad || !on ? -1 : (valid && lab == 0 ? 0 : s.arg);
  const int seg = on ? seg_of_row(p.offsets, p.n_segments, row) : 0;
  if (threadIdx.x == 0) {
    const int first = blockIdx.x * SEG_BLOCK, last = min(first + SEG_BLOCK, p.n_rows) - 1;
    span[0] = seg_of_row(p.offsets, p.n_segments, first);
    span[1] = seg_of_row(p.offsets, p.n_segments, last);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    for (int w = 0; w < SEG_WAVES; ++w) t += red[threadIdx.x][w];
    p.partials[(long long)blockIdx.x * 4 + threadIdx.x] = t;
  }
  const int seg_lo = span[0], seg_hi = span[1];
  if (p.n_classes <= SEG_HIST_CLASSES && seg_hi - seg_lo < SEG_HIST_SEGMENTS) {
    const int bins = p.n_classes * 3;
    for (int sg = seg_lo; sg <= seg_hi; ++sg) {                 // (work-group uniform)
      for (int i = threadIdx.x; i < bins; i += SEG_BLOCK) hist[i] = 0;
      __syncthreads();
      if (on && seg == sg) {
        if (gt_c >= 0) atomicAdd(&hist[gt_c * 3 + 1], 1);
        if (pr_c >= 0) atomicAdd(&hist[pr_c * 3 + 2], 1);
        if (gt_c >= 0 && gt_c == pr_c) atomicAdd(&hist[gt_c * 3], 1);
      }
      __syncthreads();
      int* __restrict__ out = p.counts + (long long)sg * bins;
      for (int i = threadIdx.x; i < bins; i += SEG_BLOCK) {
        const int h = hist[i];
        if (h) atomicAdd(out + i, h);
      }
      __syncthreads();
    }
  } else if (on) {
    int* __restrict__ out = p.counts + (long long)seg * p.n_classes * 3;
    if (gt_c >= 0) atomicAdd(out + gt_c * 3 + 1, 1);
    if (pr_c >= 0) atomicAdd(out + pr_c * 3 + 2, 1);
    if (gt_c >= 0 && gt_c == pr_c) atomicAdd(out + gt_c * 3, 1);
  }
}

// stats[0] = mean loss over the counted rows (0 / 0 = nan when there are none, like nn.CrossEntropyLoss with every row
// ignored), stats[1] = counted rows, stats[2] = correct rows, stats[3] = bad rows
__global__ __launch_bounds__(256) void csn_ragged_seg_finish_kernel(const double* __restrict__ partials, long long n_blocks,
                                                                    double* __restrict__ out) {
  __shared__ double red[4][256];
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < n_blocks; i += 256)
    for (int k = 0; k < 4; ++k) a[k] += partials[i * 4 + k];
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = red[0][0] / red[1][0];
    out[1] = red[1][0];
    out[2] = red[2][0];
    out[3] = red[3][0];
  }
}

// One work-group per 256 rows.  FLAT (ld == dld == n_classes, 16-byte aligned bases): the rows are one contiguous run on both
// sides, 16-byte accesses; otherwise one element per access, any pitch and alignment.  Only the columns [0, n_classes) of a
// gradient row are written.
template <bool FLAT>
__global__ __launch_bounds__(SEG_BLOCK) void csn_ragged_seg_bwd_kernel(CsnRaggedSegArgs p) {
  __shared__ float s_lse[SEG_BLOCK];
  __shared__ float s_nll[SEG_BLOCK];
  __shared__ int s_lab[SEG_BLOCK];                              // the label of a counted row, -1 otherwise
  const int row0 = blockIdx.x * SEG_BLOCK;
  const int rows = min(SEG_BLOCK, p.n_rows - row0);
  const int nc = p.n_classes;
  if ((int)threadIdx.x < rows) {
    const long long lab = p.labels[row0 + threadIdx.x];
    s_lse[threadIdx.x] = p.lse[row0 + threadIdx.x];
    s_nll[threadIdx.x] = p.nll[row0 + threadIdx.x];
    s_lab[threadIdx.x] = lab >= 0 && lab < nc && lab != p.ignore_label ? (int)lab : -1;
  }
  __syncthreads();
  const float scale = (float)((double)p.grad_out[0] / p.stats[1]);
  const csn_rsrc_t src = csn_make_rsrc(p.logits + (long long)row0 * p.ld, ((long long)(rows - 1) * p.ld + nc) * 4);
  const csn_rsrc_t dst = csn_make_rsrc(p.dlogits + (long long)row0 * p.dld, ((long long)(rows - 1) * p.dld + nc) * 4);
  auto grad = [&](float z, int r, int c) {
    const int lab = s_lab[r];
    if (lab < 0) return 0.f;
    // a logit of -inf is a probability of zero; the label's entry p - 1 = -(1 - exp(-nll)) without the cancellation
    const float d = c == lab ? expm1f(-s_nll[r]) : (z == -INFINITY ? 0.f : expf(z - s_lse[r]));
    return d * scale;
  };
  const int total = rows * nc;
  if constexpr (FLAT) {
    int f = threadIdx.x * 4, r = f / nc, c = f - r * nc;
    const int dr = (SEG_BLOCK * 4) / nc, dc = SEG_BLOCK * 4 - dr * nc;
    for (; f < total; f += SEG_BLOCK * 4) {
      if (f + 3 < total) {
        const f32x4 z = csn_bload4(src, (unsigned)f * 4u);
        f32x4 d;
        int rr = r, cc = c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d[e] = grad(z[e], rr, cc);
          if (++cc == nc) { cc = 0; ++rr; }
        }
        csn_bstore4(d, dst, (unsigned)f * 4u);
      } else {
        int rr = r, cc = c;
        for (int e = 0; e < 4 && f + e < total; ++e) {
          csn_bstore(grad(csn_bload(src, (unsigned)(f + e) * 4u), rr, cc), dst, (unsigned)(f + e) * 4u);
          if (++cc == nc) { cc = 0; ++rr; }
        }
      }
      r += dr; c += dc;
      if (c >= nc) { c -= nc; ++r; }
    }
  } else {
    int r = threadIdx.x / nc, c = threadIdx.x - r * nc;
    const int dr = SEG_BLOCK / nc, dc = SEG_BLOCK - dr * nc;
    for (int f = threadIdx.x; f < total; f += SEG_BLOCK) {
      const float z = csn_bload(src, (unsigned)(r * p.ld + c) * 4u);
      csn_bstore(grad(z, r, c), dst, (unsigned)(r * p.dld + c) * 4u);
      r += dr; c += dc;
      if (c >= nc) { c -= nc; ++r; }
    }
  }
}

}  // namespace

long long csn_ragged_seg_blocks(int n_rows) { return ((long long)n_rows + SEG_BLOCK - 1) / SEG_BLOCK; }

int csn_launch_ragged_seg_fwd(const CsnRaggedSegArgs& a0, hipStream_t st) {
  CsnRaggedSegArgs a = a0;
  const int cols = a.ld <= SEG_COLS ? a.ld : SEG_COLS;
  a.pitch = cols | 1;
  a.vec = a.ld <= SEG_COLS && !(reinterpret_cast<uintptr_t>(a.logits) & 15);   // (a chunk starts 256 ld bytes into the run)
  const long long blocks = csn_ragged_seg_blocks(a.n_rows);
  hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.n_segments * a.n_classes * 3 * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const size_t lds = (size_t)SEG_WAVES * SEG_ROWS * a.pitch * sizeof(float);
  hipLaunchKernelGGL(csn_ragged_seg_fwd_kernel, dim3((unsigned)blocks), dim3(SEG_BLOCK), lds, st, a);
  hipLaunchKernelGGL(csn_ragged_seg_finish_kernel, dim3(1), dim3(256), 0, st, a.partials, blocks, a.stats);
  return (int)hipGetLastError();
}

int csn_launch_ragged_seg_bwd(const CsnRaggedSegArgs& a, hipStream_t st) {
  const long long blocks = csn_ragged_seg_blocks(a.n_rows);
  const bool flat = a.ld == a.n_classes && a.dld == a.n_classes && !(reinterpret_cast<uintptr_t>(a.logits) & 15) &&
                    !(reinterpret_cast<uintptr_t>(a.dlogits) & 15);
  if (flat) hipLaunchKernelGGL(csn_ragged_seg_bwd_kernel<true>, dim3((unsigned)blocks), dim3(SEG_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(csn_ragged_seg_bwd_kernel<false>, dim3((unsigned)blocks), dim3(SEG_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}
