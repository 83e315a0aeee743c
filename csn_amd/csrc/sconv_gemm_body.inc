// The body of the gather-GEMM kernels of sparse_conv.hip, included into sconv_gemm_kernel (MODE 0 fp32 / 1 bf16x3) and
// sconv_gemm16_kernel (MODE 2 bf16 / 3 fp16: one product, the tile holds shorts) with NB, MODE, B_KN, BN, ACC and the argument p in
// scope.  ACC (sconv_gemm_acc_kernel, sparse_conv_cat.hip: a later launch of a chain over the parts of a concatenation) adds the z that
// is already in c to the accumulators before store_tile, so that the stored sum and its statistics are the chain's.
// BN (sconv_gemm_bn_kernel / sconv_gemm16_bn_kernel: forward instances, p a SconvBnP) takes the BatchNorm + residual + ReLU epilogue
// of store_tile_bn in place of store_tile.  The loop is the same text either way: the same sums in the same order.
// It is text and not a __device__ function on purpose: called through a function (by reference, by value or field by field) the
// fp32 NB = 4 dx instance takes 106 vector registers instead of 104 and loses a wave per SIMD.
  __shared__ __attribute__((aligned(16))) bs_t<MODE> Bs[NB * 32 * bs_pitch<MODE>];
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
  const csn_rsrc_t ar = csn_make_rsrc(p.a, ((long long)(p.n_src - 1) * p.lda + p.K) * 4LL);
  const unsigned a_in = (unsigned)((MODE == 0 ? 4 : 8) * h * 4);      // byte offset of the lane's channels inside a 32-channel step
  const int ks = p.K >> 5;                                            // channel steps per offset

  // the offsets at which some row of the tile has a neighbour, in ascending order
  for (int k = tid; k < p.KV; k += 256) s_flag[k] = 0;
  __syncthreads();
  for (int k = 0; k < p.KV; ++k) {
    const int r = row_ok ? p.table[(long long)(p.rev ? p.KV - 1 - k : k) * p.M + row_l] : -1;
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
    const int k = s_act[s / ks];
    return p.table[(long long)(p.rev ? p.KV - 1 - k : k) * p.M + row_l];
  };
  f32x4 an[4], bn[NB];
  auto load_a = [&](int s, int src) {
    const unsigned off = src < 0 ? CSN_OOB : (unsigned)src * (unsigned)p.lda * 4u + a_in + (unsigned)((s % ks) * 128);
#pragma unroll
    for (int g = 0; g < 4; ++g) an[g] = csn_bload4(ar, off + (unsigned)(a_kofs<MODE>(g) * 4));
  };
  auto load_w = [&](int s) {
    load_b<NB, B_KN>(bn, p.b + (long long)s_act[s / ks] * p.c_in * p.c_out, p.c_out, (s % ks) * 32, j0, p.J, tid);
  };

  int r1 = row_of(0);
  if (S > 0) { load_a(0, r1); load_w(0); }
  r1 = row_of(1);
  int r2 = row_of(2);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                                                  // the previous step's reads of Bs are done
    store_b<NB, B_KN, MODE>(Bs, bn, tid);
    f32x4 af[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = an[g];
    __syncthreads();
    if (s + 1 < S) { load_a(s + 1, r1); load_w(s + 1); }
    r1 = r2;
    r2 = row_of(s + 3);
    mma_step<NB, MODE>(acc, af, Bs, li, h);
  }

  const long long row_w = row_g + wave * 32;                          // first row of the wave's tile
  const int cnt = (int)(p.M - row_w < 32 ? (p.M - row_w < 0 ? 0 : p.M - row_w) : 32);
  // BN: the epilogue's arguments are read from the kernel-argument segment here, after the loop (bn_args_late, sparse_conv.hip)
  [[maybe_unused]] const auto* q = [&] { if constexpr (BN) return bn_args_late(); else return &p; }();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = j0 + nb * 32 + li;
    if (j0 + nb * 32 >= p.J) continue;                                // wave-uniform: J % 32 == 0
    if constexpr (BN) {
      // the lane's column of the block: its two constants, formed here from the four vectors (no preparation launch)
      const float sc = q->gamma[col] / sqrtf(q->rvar[col] + q->eps);
      store_tile_bn(acc[nb], sc, q->beta[col] - q->rmean[col] * sc, q->r, q->ldr, q->relu != 0, p.c, p.ldc, row_w, cnt, col, h);
    } else {
      if constexpr (ACC) {
        // the sum of the parts before this one: z is read where store_tile writes it, each element by the lane that stores it
        const float* cw = p.c + row_w * p.ldc;
        const int lane = 4 * h * p.ldc + col;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (csn_acc_row(r, h) < cnt) acc[nb][r] += (cw + csn_acc_row(r, 0) * p.ldc)[lane];
      }
      store_tile(acc[nb], p.bias ? p.bias[col] : 0.f, p.c, p.ldc, row_w, cnt, col, h, p.part != nullptr, p.part, (long long)rg * 4 + wave,
                 p.J);
    }
  }
