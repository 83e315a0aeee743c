// The body of the one-weight octant product of octant_conv.hip, included into octant_rows_kernel (p an OctRowsP) and
// octant_rows_bn_kernel (p an OctRowsBnP: the up convolution's forward with the inference epilogue) with NB, MODE, B_KN, BN, STATS and
// the argument p in scope.  BN stores act(acc * s + t + r) through the same destinations in place of acc + bias.  STATS
// (octant_conv_stats.hip, p an OctRowsStatsP) stores acc + bias and then forms the (mean, M2) of the wave's rows with their count.
// The loop is the same text in every form: the same sums in the same order.  Text and not a __device__ function, as
// sconv_gemm_body.inc is and for its reason.
  __shared__ __attribute__((aligned(16))) float Bs[NB * 32 * BS_PITCH];
  __shared__ int s_dst[128];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  // STATS: the epilogue's own arguments (part, cnt) are reached through a pointer of the instance's argument type, as q below
  [[maybe_unused]] const auto* sq = [&] { return &p; }();
  int k, lo, hi;
  if (!octant_span(p.seg, p.M, rg, 128, k, lo, hi)) {                 // uniform over the work-group
    if constexpr (STATS) {
      if (cg == 0 && tid < 4) sq->cnt[rg * 4 + tid] = 0;                // its four wave tiles hold no rows
    }
    return;
  }
  const int r = lo + wave * 32 + li;                                  // the lane's entry of `order`
  int dst = r < hi ? p.order[r] : -1;
  if (dst >= p.M) dst = -1;
  int src = dst >= 0 ? p.parent[dst] : -1;
  if (src >= p.n_src) src = -1;
  if (h == 0) s_dst[wave * 32 + li] = dst;
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * 4LL);
  const unsigned a_row = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 4u + (unsigned)((MODE == 0 ? 4 : 8) * h * 4);
  const float* bk = p.b + (long long)k * p.c_in * p.c_out;
  const int S = p.K >> 5;                                             // 32-channel steps

  f32x16 acc[NB] = {};
  f32x4 an[4], bn[NB];
  auto load = [&](int s) {
    const unsigned off = src < 0 ? CSN_OOB : a_row + (unsigned)(s * 128);
#pragma unroll
    for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, off + (unsigned)(a_kofs<MODE>(g) * 4));
    load_b<NB, B_KN>(bn, bk, p.c_out, s * 32, j0, p.J, tid);
  };
  load(0);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, B_KN, MODE>(Bs, bn, tid);
    f32x4 af[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) load(s + 1);
    mma_step<NB, MODE>(acc, af, Bs, li, h);
  }

  // the wave's 32 rows leave for their own places: accumulator row rr of the lane goes to row s_dst[rr], 32 lanes one 128-byte run
  const csn_rsrc_t cr = csn_make_rsrc(p.c, ((long long)(p.M - 1) * p.ldc + p.J) * 4LL);
  // BN: the epilogue's arguments are read from the kernel-argument segment here, after the loop (oct_bn_args_late, octant_conv.hip)
  [[maybe_unused]] const auto* q = [&] { if constexpr (BN) return oct_bn_args_late(); else return &p; }();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    const int col = j0 + nb * 32 + li;
    if constexpr (BN) {
      // the lane's column of the block: its two constants, formed here from the four vectors (store_tile_bn's arithmetic); the
      // residual goes through a descriptor of its own pitch, each element read and then written by the same lane (r may be c)
      const float sc = q->gamma[col] / sqrtf(q->rvar[col] + q->eps);
      const float sh = q->beta[col] - q->rmean[col] * sc;
      const float* rp = q->r;
      const int ldr = q->ldr;
      const bool relu = q->relu != 0;
      const csn_rsrc_t rr = csn_make_rsrc(rp, rp ? ((long long)(p.M - 1) * ldr + p.J) * 4LL : 0LL);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int d = s_dst[wave * 32 + csn_acc_row(e, h)];
        float v = fmaf(acc[nb][e], sc, sh);
        if (rp) v += csn_bload(rr, d < 0 ? CSN_OOB : ((unsigned)d * (unsigned)ldr + (unsigned)col) * 4u);
        csn_bstore(relu ? fmaxf(0.f, v) : v, cr, d < 0 ? CSN_OOB : ((unsigned)d * (unsigned)p.ldc + (unsigned)col) * 4u);
      }
    } else {
      const float bv = p.bias ? p.bias[col] : 0.f;
      [[maybe_unused]] unsigned live = 0;                               // STATS: bit e set where accumulator row e has a destination
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int d = s_dst[wave * 32 + csn_acc_row(e, h)];
        if constexpr (STATS) live |= (d >= 0 ? 1u : 0u) << e;
        csn_bstore(acc[nb][e] + bv, cr, d < 0 ? CSN_OOB : ((unsigned)d * (unsigned)p.ldc + (unsigned)col) * 4u);
      }
      if constexpr (STATS) {
        // (mean, M2) of the column over the wave's rows that have a destination — 0 to 32 of them, counted and not assumed —
        // in two passes over the registers (store_tile's arithmetic); the count goes beside them once per tile
        const int cnt = __popcll(__ballot(h == 0 && dst >= 0));
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (live >> e & 1u) sum += acc[nb][e] + bv;
        sum += csn_xhalf(sum);
        const float mu = cnt > 0 ? sum / (float)cnt : 0.f;
        float m2 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float dv = (acc[nb][e] + bv) - mu;
          if (live >> e & 1u) m2 = fmaf(dv, dv, m2);
        }
        m2 += csn_xhalf(m2);
        const int tile = rg * 4 + wave;                                 // < (ceil(M / 128) + 7) * 4, the rows of part and cnt
        const csn_rsrc_t pr = csn_make_rsrc(sq->part, (((long long)p.M + 127) / 128 + 7) * 4 * 2 * p.J * 4LL);
        const unsigned po = h == 0 ? ((unsigned)(tile * 2) * (unsigned)p.J + (unsigned)col) * 4u : CSN_OOB;
        csn_bstore(mu, pr, po);
        csn_bstore(m2, pr, h == 0 ? po + (unsigned)p.J * 4u : CSN_OOB);
        if (cg == 0 && nb == 0 && l == 0) sq->cnt[tile] = cnt;
      }
    }
  }
