// dV of the kept-scores attention backward, formed FROM THE SCORES: dV^T[c][key] = sum_q dO^T[c][q] P_drop[q][key] with
// P_drop = exp(S - lse) mask / (1 - p) rebuilt in registers from the forward's S, its lse and the masks' seed (autograd of
// ScaledDotProductAttention.forward, MID-FC/csa_models.py:138-144, w.r.t. v).  The dQ kernel (attn_bf16x3.hip, NOP instance) then
// neither splits P nor writes it over S, and the plane product that read those planes back is not run for dV: the dQ launch writes 4 T Tp
// bytes per score block less, and this kernel reads S where the product read P (DESIGN.md section 4x, item (11) revisited).
//
// The skeleton is the key-stationary kernel of attn_dkv.hip without its first phase: a work-group of 8 waves owns 128 keys of one
// (key/value slot, head, block); wave w holds the accumulators dV^T[d][16 keys] of its keys (d = 256: 64 registers) and the
// work-group streams, for every evaluation that reads this slot, 32-query tiles of
//   S    [32 queries][128 keys] fp32 — whole 512-byte row segments (tile-major scores: four 128-byte tile rows), 16-byte
//        pieces, through LDS (a lane then picks the 8
//        consecutive queries of its key: chunk c of row r sits at c ^ 4 ((r >> 3) & 1), so the two lane quarters that share a
//        32-lane read group use complementary banks);
//   dO^T [d][32 queries] fp32 — split into bf16 hi / lo once per tile and work-group, into the query-contiguous image of
//        attn_dkv.hip's second phase (16-byte fragment reads);
//   lse  32 values, scaled by log2(e) once.
// Per tile and lane: P of its key against 8 consecutive queries — the same exp2(S log2e - lse log2e), the same csn_pair_hash over
// the same pair index and salt and the same 1 / (1 - p) as the dQ kernel; one hash per key pair, shared by the two neighbouring
// lanes that hold the pair — split into hi / lo in registers: the B fragment of the product as it stands, no LDS round trip.
// Tails.  Queries beyond the block end: their pieces of S, dO and lse are switched off in the requests (zeros), so P = 1 meets a
// zero row of dO.  Keys beyond the block end (T % 4 == 0: a piece is all in or all out): S reads as zero and P is set to zero;
// a key is a COLUMN of the product, and the epilogue stores nothing beyond the block's keys.
// Schedule: two stages of every image, ONE barrier per tile: in step t a wave commits tile t + 1 (requested in step t - 1) to
// the other stage, requests tile t + 2 and computes tile t.  Waves 0..3 commit first and compute after, waves 4..7 — their SIMD
// partners — compute first: a SIMD has one wave in the matrix segment beside one in its vector work.
// Occupancy: the two-wave bound (256 registers, no scratch).  The tile images — 64 KB of dO^T planes and 32 KB of S — leave no
// room for a second work-group on the CU, so the four-wave bound would buy nothing.
#include "csn_common.h"
#include "csn_kernels.h"

namespace {

constexpr int QT = 32;               // queries per streamed tile
constexpr int KW = 128;              // keys per work-group: 16 per wave
constexpr float LOG2E = 1.4426950408889634f;

using namespace csn_mode;
typedef f32x4m f32x4v;
typedef short __attribute__((address_space(3))) lds_s16;
typedef s16x8 __attribute__((address_space(3))) lds_s16x8;

CSN_DEVINL const lds_s16* opaque_lds(const short* p) {
  const lds_s16* q = (const lds_s16*)p;
  asm volatile("" : "+v"(q));
  return q;
}

template <typename PR>
CSN_DEVINL f32x4v mma16(s16x8 ah, s16x8 al, s16x8 bh, s16x8 bl, f32x4v c) {
  c = mfma16<PR::HALF>(al, bh, c);                    // small terms first
  c = mfma16<PR::HALF>(ah, bl, c);
  return mfma16<PR::HALF>(ah, bh, c);
}

// DR: dropout live (a compile-time property, as in attn_dkv.hip)
template <typename PR, int DT, bool DR>
__global__ __launch_bounds__(512, 2) void csn_attn_dv_scores_kernel(CsnAttnDvArgs p) {
  static_assert(PR::NT == 3 && PR::NPL == 2, "two planes, three products");
  constexpr int NT = 512;
  constexpr int D = 32 * DT;
  constexpr int PLANE = D * QT + 32;                    // hi and lo planes 64 bytes out of phase (store banks, attn_bf16x3.hip)
  constexpr int NP_O = D * 8 / NT;                      // 16-byte pieces of a [D][32] fp32 tile per thread
  constexpr int NP_S = QT * (KW / 4) / NT;              // ... of a [32][128] fp32 tile: 2
  constexpr int NST = 2;                                // stages
  constexpr int IMG_EL = NST * 2 * PLANE;               // shorts: dO^T [stage][plane]
  constexpr int S_EL = QT * KW;                         // floats of one S stage
  constexpr int ER = D < 128 ? D : 128;                 // rows per pass of the epilogue's transpose block (it lies over the images)
  static_assert((D * 8) % NT == 0 && D % ER == 0 && ER * KW * 2 <= IMG_EL, "tile pieces fill the passes; the transpose block fits the images");
  __shared__ __attribute__((aligned(16))) short tiles[IMG_EL + NST * S_EL * 2 + NST * QT * 2];
  auto image = [&](int st, int pl) -> short* { return tiles + (st * 2 + pl) * PLANE; };
  float* sbuf = reinterpret_cast<float*>(tiles + IMG_EL);             // [stage][32 queries][128 keys]
  float* lbuf = sbuf + NST * S_EL;                                    // [stage][32]: lse log2(e)
  float* xbuf = reinterpret_cast<float*>(tiles);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, kq = lane >> 4;
  // XCD-aware order (attn_dkv.hip): the KC key chunks of a unit stream the same dO tiles — same residue mod 8
  const int KC = (p.T + KW - 1) / KW;
  const int Y = p.n_blocks * p.H;
  const int L = blockIdx.x, slot8 = L & 7, jj = L >> 3;
  const int kc = jj % KC, u = (jj / KC) * 8 + slot8;
  if (u >= Y * p.n_groups) return;
  const int grp = u / Y, hd = (u % Y) % p.H, blk = (u % Y) / p.H;
  const int it0 = p.grp_off ? p.grp_off[grp] : grp, it1 = p.grp_off ? p.grp_off[grp + 1] : grp + 1;
  const bool short_blk = p.T_last > 0 && blk == p.n_blocks - 1;
  const int e_first = p.eval_ids ? p.eval_ids[it0] : it0;
  const int T = short_blk ? p.T_last : p.T;                         // queries = keys of this block
  if (kc * KW >= T) return;
  const int QL = p.T;                                               // queries per block that lay out the maps, the scores and the statistics
  const int ld = p.ld, Tp = p.Tp;
  const bool tile_major = p.sc_layout != 0;
  const int nk = T - kc * KW;                                       // keys of this chunk that exist (a multiple of 4)
  const int nkc = nk < KW ? nk : KW;
  const int nqt = (T + QT - 1) / QT;
  const int n_steps = (it1 - it0) * nqt;
  const bool late = __builtin_amdgcn_readfirstlane(wave) >= 4;
  const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
  const int col0 = 16 * wave + lq;                                  // this lane's key inside the chunk
  const int key0 = kc * KW + col0;                                  // ... inside the block
  const bool key_ok = key0 < T;

  f32x4v dV[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) dV[c] = f32x4v{0.f, 0.f, 0.f, 0.f};

  const unsigned thr16 = csn_drop_threshold16(p.dropout_p);
  const float keep_scale = DR ? 1.f / (1.f - p.dropout_p) : 1.f;
  const int mp = QL > Tp ? QL : Tp;                                 // mask pitch of the forward (queries per block vs score pitch)
  const unsigned pw_key = (unsigned)((key0 >> 1) * mp);             // pair index of this lane's key: (key / 2) * mp + query
  const bool key_odd = key0 & 1;

  // ---- streamed tiles -------------------------------------------------------------------------------------------
  // dO^T: 16-byte piece t_c of row t_row (+ 64 i); S: piece s_c (keys 4 s_c ..) of query row s_row (+ 16 i)
  const int t_c = tid & 7, t_row = tid >> 3;
  const int t_swz = (-((t_row >> 2) & 3)) & 3;
  const int b_dst = t_row * QT + 8 * ((t_c >> 1) ^ t_swz) + 4 * (t_c & 1);
  const int s_c = tid & 31, s_row = tid >> 5;
  const int s_dst = s_row * KW + ((s_c ^ (4 * ((s_row >> 3) & 1))) << 2);
  f32x4 gO[NP_O], gS[NP_S];
  float gl = 0.f;
  int f_it = it0, f_qt = 0;                                         // fetch stream: (item, query tile) of the next tile to request
  csn_rsrc_t Or_it, Sr_it, Lr_it;
  auto fetch_item = [&]() __attribute__((always_inline)) {
    const int e = p.eval_ids ? p.eval_ids[f_it] : f_it;
    const long long unit = (long long)e * p.H + hd;
    const long long head_off = (long long)hd * D * ld + (long long)blk * QL;
    Or_it = csn_make_rsrc(p.dctx + (long long)e * p.ctx_eval_stride + head_off, ((long long)(D - 1) * ld + T) * 4);
    // window of the scores: rows 0 .. T - 1 of this block, the chunk's existing keys of the last row (tile-major: the block)
    const float* sblk = p.scores + (unit * p.n_blocks + blk) * ((long long)QL * Tp);
    Sr_it = tile_major ? csn_make_rsrc(sblk, (long long)QL * Tp * 4) : csn_make_rsrc(sblk + kc * KW, ((long long)(T - 1) * Tp + nkc) * 4);
    Lr_it = csn_make_rsrc(p.lse + unit * ((long long)p.n_blocks * QL) + (long long)blk * QL, (long long)T * 4);
  };
  fetch_item();
  // this thread's piece of the S tile: row-major [query][key] of pitch Tp, or tile-major [key tile][query of QL][32 keys]
  const unsigned s_lane = tile_major ? (unsigned)(((kc * (KW / 32) + (s_c >> 3)) * QL + s_row) * 32 + 4 * (s_c & 7)) * 4u
                                     : (unsigned)(s_row * Tp + 4 * s_c) * 4u;
  const unsigned s_rows16 = tile_major ? 16u * 32u * 4u : (unsigned)(16 * Tp) * 4u;       // bytes from query q to q + 16
  const unsigned s_row1 = tile_major ? 32u * 4u : (unsigned)Tp * 4u;                      // ... to q + 1
  const unsigned t_off = (unsigned)(t_row * ld + 4 * t_c) * 4u;
  auto fetch = [&]() __attribute__((always_inline)) {
    const int q_first = f_qt * QT;                                  // first query of the tile inside the block
    // (the hardware range check does not see scalar offsets: queries beyond the block end are switched off in the lane offset)
    const unsigned off = (q_first + 4 * t_c) < T ? t_off : CSN_OOB; // T % 4 == 0: a piece is all in or all out
#pragma unroll
    for (int i = 0; i < NP_O; ++i) gO[i] = csn_bload4(Or_it, off, (unsigned)(q_first + 64 * i * ld) * 4u);
#pragma unroll
    for (int i = 0; i < NP_S; ++i) {
      const bool ok = (q_first + s_row + 16 * i) < T && 4 * s_c < nk;
      gS[i] = csn_bload4_stream(Sr_it, ok ? s_lane + (unsigned)i * s_rows16 : CSN_OOB, (unsigned)q_first * s_row1);
    }
    if (wave0) gl = csn_bload(Lr_it, lane < 32 ? (unsigned)(q_first + lane) * 4u : CSN_OOB);   // (beyond the block: 0, by the range check)
    if (++f_qt == nqt) {                                            // next tile: the first of the next item (if any)
      f_qt = 0;
      if (++f_it < it1) fetch_item();
    }
  };
  auto commit = [&](int st) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NP_O; ++i) {
      s16x4 hi, lo;
      split4<PR>(gO[i], hi, lo);
      *reinterpret_cast<s16x4*>(image(st, 0) + b_dst + 64 * QT * i) = hi;
      *reinterpret_cast<s16x4*>(image(st, 1) + b_dst + 64 * QT * i) = lo;
    }
#pragma unroll
    for (int i = 0; i < NP_S; ++i) *reinterpret_cast<f32x4*>(&sbuf[st * S_EL + s_dst + 16 * KW * i]) = gS[i];
    if (wave0 && lane < 32) lbuf[st * QT + lane] = gl * LOG2E;
  };

  // fragment read position of the product (attn_dkv.hip, phase 2): row lq of the 16-channel tile, queries 8 kq .. 8 kq + 7
  const int b_pos = lq * QT + 8 * (kq ^ ((-((lq >> 2) & 3)) & 3));
  // this lane's scores: rows 8 kq + j, column col0
  const int s_pos = 8 * kq * KW + ((((col0 >> 2) ^ (4 * (kq & 1))) << 2) | (col0 & 3));

  constexpr int NC = D / 16, PD = 4;                                // fragment ring: reads run PD steps ahead of the matrix instructions
  auto compute = [&](int st, int c_qt, unsigned salt) __attribute__((always_inline)) {
    const lds_s16* tOh = opaque_lds(image(st, 0) + b_pos);
    s16x8 voh[PD], vol[PD];
#pragma unroll
    for (int c = 0; c < PD; ++c) {                                  // the first fragments land under the pointwise segment
      voh[c] = *reinterpret_cast<const lds_s16x8*>(tOh + c * 16 * QT);
      vol[c] = *reinterpret_cast<const lds_s16x8*>(tOh + PLANE + c * 16 * QT);
    }
    const f32x4 l0 = *reinterpret_cast<const f32x4*>(&lbuf[st * QT + 8 * kq]), l1 = *reinterpret_cast<const f32x4*>(&lbuf[st * QT + 8 * kq + 4]);
    const float lse2[8] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    float sv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sv[j] = sbuf[st * S_EL + s_pos + j * KW];
    const int q0 = c_qt * QT + 8 * kq;                              // first of this lane's 8 queries (inside the block)
    // one mixer round decides the two keys of a pair, and they sit on neighbouring lanes: the even lane hashes queries 0..3, the
    // odd lane 4..7, and a quad swap hands each the other's four (attn_dkv.hip)
    unsigned hsh[8];
    if constexpr (DR) {
      unsigned mine[4], theirs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) mine[j] = csn_pair_hash(pw_key + (unsigned)(q0 + (key_odd ? 4 : 0) + j), salt);
#pragma unroll
      for (int j = 0; j < 4; ++j) theirs[j] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine[j], 0xB1, 0xf, 0xf, false);   // lane ^ 1
#pragma unroll
      for (int j = 0; j < 4; ++j) { hsh[j] = key_odd ? theirs[j] : mine[j]; hsh[4 + j] = key_odd ? mine[j] : theirs[j]; }
    }
    s16x8 ph, pl;                                                   // P_drop of the tile as the product's B fragment
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float pv = __builtin_amdgcn_exp2f(fmaf(sv[r], LOG2E, -lse2[r]));   // softmax probability (csa_models.py:141)
      bool keep = true;
      if constexpr (DR) keep = (key_odd ? (hsh[r] >> 16) : (hsh[r] & 0xffffu)) >= thr16;
      const float md = keep ? keep_scale : 0.f;
      const float pd = key_ok ? pv * md : 0.f;                      // keys beyond the block end
      ph[r] = to16<PR::HALF>(pd);
      pl[r] = to16<PR::HALF>(pd - from16<PR::HALF>(ph[r]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int r = c % PD;
      dV[c] = mma16<PR>(voh[r], vol[r], ph, pl, dV[c]);
      if (c + PD < NC) {
        voh[r] = *reinterpret_cast<const lds_s16x8*>(tOh + (c + PD) * 16 * QT);
        vol[r] = *reinterpret_cast<const lds_s16x8*>(tOh + PLANE + (c + PD) * 16 * QT);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  fetch();
  commit(0);
  if (n_steps > 1) fetch();
  __syncthreads();

  int c_it = it0, c_qt = 0;                                         // (item, query tile) of the product
  unsigned salt = 0;
  for (int step = 0; step < n_steps; ++step) {
    const int cur = step & 1, nxt = cur ^ 1;
    const bool more = step + 1 < n_steps;
    if (c_qt == 0) {                                                // a new item: its mask salt (scalar unit)
      const int e = p.eval_ids ? p.eval_ids[c_it] : c_it;
      salt = csn_block_salt((unsigned long long)(((long long)e * p.H + hd) * p.n_blocks + blk), p.seed);
    }
    // stage nxt was last read in step - 1, behind that step's barrier
    if (!late && more) { commit(nxt); if (step + 2 < n_steps) fetch(); }
    compute(cur, c_qt, salt);
    if (late && more) { commit(nxt); if (step + 2 < n_steps) fetch(); }
    if (++c_qt == nqt) { c_qt = 0; ++c_it; }
    __syncthreads();
  }

  // ---- epilogue: dV^T [d][128 keys] leaves as 16-byte rows through an LDS transpose, ER rows per pass ------------------
  const int cc = tid & 31, crow = tid >> 5;                         // 4-key chunk of the row, first row (+ 16 t)
  constexpr int CH_T = ER / 16;
  const long long ovslot = p.dv_index ? p.dv_index[e_first] : e_first;
  const long long out_off = (long long)hd * D * ld + (long long)blk * p.T + kc * KW;
  const csn_rsrc_t rs = csn_make_rsrc(p.dv + ovslot * p.dkv_slot_stride + out_off, ((long long)(D - 1) * ld + nkc) * 4);
  const unsigned c_off = (4 * cc) < nk ? (unsigned)(crow * ld + 4 * cc) * 4u : CSN_OOB;
#pragma unroll
  for (int h = 0; h < D / ER; ++h) {
    if (h) __syncthreads();
#pragma unroll
    for (int c = 0; c < ER / 16; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * c + 4 * kq + r;
        xbuf[row * KW + ((((col0 >> 2) ^ (4 * ((row >> 2) & 1))) << 2) | (col0 & 3))] = dV[h * (ER / 16) + c][r];
      }
    __syncthreads();
    f32x4 ch[CH_T];
#pragma unroll
    for (int t = 0; t < CH_T; ++t) {
      const int row = crow + 16 * t;
      ch[t] = *reinterpret_cast<const f32x4*>(&xbuf[row * KW + ((cc ^ (4 * ((row >> 2) & 1))) << 2)]);
    }
#pragma unroll
    for (int t = 0; t < CH_T; ++t) csn_bstore4(ch[t], rs, c_off, (unsigned)((h * ER + 16 * t) * ld) * 4u);
  }
}

template <typename PR, int DT>
int launch_dt(const CsnAttnDvArgs& a, hipStream_t st) {
  const long long units = (long long)a.n_blocks * a.H * a.n_groups;
  const int KC = (a.T + KW - 1) / KW;
  dim3 grid((unsigned)(((units + 7) / 8) * 8 * KC));
  if (a.dropout_p > 0.f) hipLaunchKernelGGL((csn_attn_dv_scores_kernel<PR, DT, true>), grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL((csn_attn_dv_scores_kernel<PR, DT, false>), grid, dim3(512), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

int csn_launch_attn_dv_scores(const CsnAttnDvArgs& a, int d, int mode, hipStream_t st) {
  if (a.n_groups <= 0 || a.n_blocks <= 0) return 0;
  if (mode != 1 || !csn_attn_dv_scores_fits(mode, d)) return -1;
  if ((a.ld & 3) || (a.T & 3) || (a.T_last & 3) || (a.Tp & 3) || a.T > 512 || a.Tp < a.T) return -2;
  if (a.sc_layout && a.Tp < (a.T + 31) / 32 * 32) return -2;         // tile-major: whole 32-key tiles
  if ((a.ctx_eval_stride & 3) || (a.dkv_slot_stride & 3)) return -4;
  // lane offsets are 32-bit byte offsets into windows below 2 GiB (csn_common.h)
  if ((long long)d * a.ld * 4 >= 0x7fffffffLL || (long long)a.T * a.Tp * 4 >= 0x7fffffffLL) return -2;
  return launch_dt<Bf16x3, 8>(a, st);
}
