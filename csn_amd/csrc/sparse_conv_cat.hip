// The gather-GEMM of sparse_conv.hip with a BatchNorm statistics epilogue over a concatenation that is never formed
// (include/csn_hip.h section 27): z = sum_m gather-GEMM(x_m, table, W[:, c0_m : c1_m]) for 1 .. 4 parts x_m of <= 256 columns and
// ONE kernel W[kv][sum c_in][c_out] — the conv1 and the downsample convolution of a Res16UNet decoder block that reads more than
// 256 columns.  Part m's weights are rows [c0_m, c1_m) of every W[k]: the product reaches them through a base offset with W's own
// strides (c_out per row, sum c_in * c_out per offset); nothing is copied or cut.
//
// A CHAIN of one launch per part:
//   part 0             sparse_conv.hip's forward as it is (w_rows: the rows of every W[k]), z = its product;
//   parts 1 ..         sconv_gemm_acc_kernel<NB, MODE>: sconv_gemm_body.inc with ACC — the same loop, and before store_tile the
//                      accumulators take up the z that the launches before left in place, each element read by the lane that
//                      stores it.  The LAST launch carries the statistics epilogue (store_tile's (mean, M2) of the completed sums),
//                      then bn_stats_merge: no pass of its own over z.
// With one part the call IS csn_launch_sparse_conv_stats_fwd.  The other form — one launch that contracts over both sources —
// was not built: it holds a buffer descriptor and a row offset per source across the loop, and the NB = 4 instances have no scalar
// or vector registers to spare (the comments at the top of sparse_conv.hip and sconv_gemm_body.inc), while the chain's extra cost
// is one read of z per later part, n_out * c_out * 4 bytes beside a gather of up to 27 * n_out * c_in * 4.
// No floating-point atomics: every sum has a fixed order, two calls give the same bits.
#include "rows_mma.h"

namespace {
using namespace rows_mma;

constexpr int MAX_KV = 27;              // the offsets this entry point takes: kernel 1 and kernel 3

struct SconvAccP {
  const float* a; int lda; int n_src;  // A[n_src][lda]: the part's map
  const int* table;                    // [KV][M]
  int rev;                             // 0 (the body's backward form is not used here)
  const float* b;                      // row c0 of W[0]
  int c_in, c_out;                     // c_in: the rows of every W[k] (sum over the parts), not the part's width K
  float* c; int ldc;                   // C[M][J]: read (the parts before), then written
  int M, K, J, KV;
  const float* bias;                   // NULL
  float* part;                         // non-NULL on the chain's last launch: the (mean, M2) of each wave's rows, [tile][2][J]
};

// named by the body's inference epilogue, which no instance here takes: declared, never defined or called
__device__ const SconvAccP* bn_args_late();

template <int NB, int MODE>
__global__ __launch_bounds__(256) void sconv_gemm_acc_kernel(const SconvAccP p) {
  constexpr bool B_KN = true, BN = NB < 0, ACC = true;
#include "sconv_gemm_body.inc"
}

template <int NB>
int launch_acc_nb(const SconvAccP& p, int mode, hipStream_t st) {
  void (*const k[4])(SconvAccP) = {sconv_gemm_acc_kernel<NB, 0>, sconv_gemm_acc_kernel<NB, 1>, sconv_gemm_acc_kernel<NB, 2>,
                                   sconv_gemm_acc_kernel<NB, 3>};
  return launch_row_product(k, p, NB, mode, st);
}

}  // namespace

// mode as csn_launch_sparse_conv_fwd; c_in[m] are the parts' widths, a.c_in their sum, a.ws csn_sparse_conv_stats_ws_bytes bytes
int csn_launch_sparse_conv_cat_stats_fwd(const CsnSparseConvArgs& a, const float* const* x, const int* ld_x, const int* c_in, int n_parts,
                                         float* mean, float* invstd, float* running_mean, float* running_var, float eps, float momentum,
                                         int mode, hipStream_t st) {
  if (n_parts == 1) {
    CsnSparseConvArgs g = a;
    g.x = x[0]; g.ld_x = ld_x[0]; g.c_in = c_in[0];
    return csn_launch_sparse_conv_stats_fwd(g, nullptr, 0, mean, invstd, running_mean, running_var, eps, momentum, mode, st);
  }
  float* part = static_cast<float*>(a.ws);
  int c0 = 0;
  for (int m = 0; m < n_parts; ++m) {
    const float* w_m = a.w + (long long)c0 * a.c_out;
    if (m == 0) {
      CsnSparseConvArgs g = a;
      g.x = x[0]; g.ld_x = ld_x[0]; g.c_in = c_in[0]; g.w = w_m; g.w_rows = a.c_in; g.bias = nullptr;
      if (const int e = csn_launch_sparse_conv_fwd(g, mode, st)) return e;
    } else {
      SconvAccP p{};
      p.a = x[m]; p.lda = ld_x[m]; p.n_src = a.n_in; p.table = a.fwd_table; p.b = w_m; p.c_in = a.c_in; p.c_out = a.c_out;
      p.c = a.y; p.ldc = a.ld_y; p.M = a.n_out; p.K = c_in[m]; p.J = a.c_out; p.KV = a.kv;
      p.part = m == n_parts - 1 ? part : nullptr;
      if (const int e = dispatch4(csn_sconv_column_blocks(p.J, p.M), [&](auto nb) { return launch_acc_nb<nb()>(p, mode, st); })) return e;
    }
    c0 += c_in[m];
  }
  const int n_tiles = (int)(((long long)a.n_out + 127) / 128) * 4;
  return csn_launch_bn_stats_merge(part, n_tiles, a.n_out, a.c_out, eps, momentum, a.y, a.ld_y, nullptr, 0, mean, invstd, running_mean,
                                   running_var, st);
}
