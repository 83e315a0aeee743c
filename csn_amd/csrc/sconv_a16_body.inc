// The contraction of the single-product gather-GEMM on a gathered map that may hold 16-bit rows, included into
// sconv_maps16_kernel (sparse_conv_maps16.hip: the inference epilogue) and sconv_stats_x16_kernel (train_maps16.hip: the statistics
// epilogue) with NB, H16, MODE, A16, MAX_KV and the argument p (a, lda, n_src, table, b, c_in, c_out, M, K, J, KV) in scope.  It is
// the loop of sconv_gemm_body.inc — the same offset list, the same walk two steps ahead, the same matrix instruction per (half step,
// column block) — with the A fragments of a 16-bit map loaded as they lie (see sparse_conv_maps16.hip); it leaves acc, j0, rg,
// row_g, wave, li and h to the epilogue.  Text and not a function for the reason given in sconv_gemm_body.inc.
  __shared__ __attribute__((aligned(16))) short Bs[NB * 32 * BS16_PITCH];
  __shared__ int s_flag[MAX_KV];
  __shared__ int s_act[MAX_KV];
  __shared__ int s_nact;
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
  const int ncg = (p.J + NB * 32 - 1) / (NB * 32);
  const int cg = blockIdx.x % ncg, rg = blockIdx.x / ncg;
  const int j0 = cg * NB * 32;
  const long long row_g = (long long)rg * 128;                        // first output row of the work-group
  const long long row_l = row_g + wave * 32 + li;                     // the lane's output row
  const bool row_ok = row_l < p.M;
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * (A16 ? 2LL : 4LL));
  const unsigned a_in = (unsigned)(A16 ? 16 * h : 32 * h);            // byte offset of the lane's channels inside a 32-channel step
  const int ks = p.K >> 5;                                            // channel steps per offset

  // the offsets at which some row of the tile has a neighbour, in ascending order
  for (int k = tid; k < p.KV; k += 256) s_flag[k] = 0;
  __syncthreads();
  for (int k = 0; k < p.KV; ++k) {
    const int r = row_ok ? p.table[(long long)k * p.M + row_l] : -1;
    if (__ballot(r >= 0) != 0ULL && l == 0) s_flag[k] = 1;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < p.KV; ++k)
      if (s_flag[k]) s_act[n++] = k;
    s_nact = n;
  }
  __syncthreads();
  const int S = s_nact * ks;                                          // contraction steps of this work-group

  f32x16 acc[NB] = {};
  // step s = (offset s / ks of the list, channels 32 (s % ks) ..): the lane's source row of a step, two steps ahead of its use
  auto row_of = [&](int s) -> int {
    if (s >= S || !row_ok) return -1;
    return p.table[(long long)s_act[s / ks] * p.M + row_l];
  };
  constexpr int NA = A16 ? 2 : 4;                                     // 16-byte reads of A per lane and step
  f32x4 an[NA], bn[NB];
  auto load_a = [&](int s, int src) {
    if constexpr (A16) {
      const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 2u + a_in + (unsigned)((s % ks) * 64);
      an[0] = csn_bload4(ar, off);
      an[1] = csn_bload4(ar, off + 32u);
    } else {
      const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 4u + a_in + (unsigned)((s % ks) * 128);
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, off + (unsigned)(a_kofs<MODE>(g) * 4));
    }
  };
  auto load_w = [&](int s) {
    load_b<NB, true>(bn, p.b + (long long)s_act[s / ks] * p.c_in * p.c_out, p.c_out, (s % ks) * 32, j0, p.J, tid);
  };

  int r1 = row_of(0);
  if (S > 0) { load_a(0, r1); load_w(0); }
  r1 = row_of(1);
  int r2 = row_of(2);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, true, MODE>(Bs, bn, tid);
    f32x4 af[NA];
#pragma unroll
    for (int g = 0; g < NA; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) { load_a(s + 1, r1); load_w(s + 1); }
    r1 = r2;
    r2 = row_of(s + 3);
    if constexpr (A16) mma_step_a16<NB, H16>(acc, af, Bs, li, h);
    else mma_step<NB, MODE>(acc, af, Bs, li, h);
  }
