// mxfp8_gemm_kernel's OUT8 instantiation (omgsr_igemm_out_mxfp8, additive under ABI v22: no struct changes): the MXFP8 x MXFP8 token GEMM whose epilogue writes the
// OMGSR_EL_MXFP8 operand of the next MXFP8 GEMM (bias + GELU-tanh of the feed-forward's first projection, proj_mlp into the single block's
// [attn | mlp] operand) instead of a bf16 tensor that omgsr_quantize_mxfp8 would read back. The codes and scale bytes are those of that
// chain: the epilogue rounds to bf16 first (igemm_epilogue.hip.h, OUT8). A translation unit of its own, like igemm_halo_out6.hip: the
// cooperative store stays out of the instantiation every other output form shares.
#include "gemm_mxfp8_body.hip.h"

namespace {
__global__ __launch_bounds__(512, 2) void mxfp8_gemm_out8_kernel(const omgsr_igemm_args p, const IgemmGeo g, const IgemmOut8 o8) {
    mxfp8_gemm_body<true>(p, g, xcd_remap(blockIdx.x, g.ntm * g.ntn), blockIdx.z, o8);
}
}  // namespace

namespace omgsr {
int mxfp8_gemm_out8_launch(const omgsr_igemm_args& a, IgemmGeo g, unsigned char* out_scale, int64_t out_scale_ld, hipStream_t st) {
    g.ntm = (g.M + BM - 1) / BM;
    g.ntn = (a.Cout + BN - 1) / BN;
    g.splits = 1;
    return launch_lds<mxfp8_gemm_out8_kernel>(dim3(g.ntm * g.ntn, 1, a.batch), dim3(512), LDS_BYTES, st, a, g, IgemmOut8{out_scale, out_scale_ld});
}
}  // namespace omgsr
