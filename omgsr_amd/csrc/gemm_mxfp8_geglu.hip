// mxfp8_gemm_kernel's GEGLU form (omgsr_igemm_geglu_mxfp8, additive under ABI v22: no struct changes): the MXFP8 x MXFP8 token GEMM of a feed-forward's
// first projection, C -> 2 x inner, whose epilogue computes (a + bias_a) * gelu(g + bias_g). The weight rows carry pack_geglu_weight's
// interleave, [32 a | 32 gate] per 64 packed columns, so a 64-wide wave tile holds both halves of 32 logical columns - exactly one MXFP8 block
// of the hidden row - and the epilogue's GEGLU branch (igemm_epilogue.hip.h) spreads a staged row over a lane quad, which is what
// mxfp8_quad_octet needs. Schedule, 256 x 256 tile and wave tiles are the body's (gemm_mxfp8_body.hip.h); the tile grid counts PACKED columns.
// Two output forms, one kernel each side of the OUT8 template flag: the plain [M][Cout] tensor (bf16 / fp32) and the OMGSR_EL_MXFP8 operand of
// net.2's GEMM (the bytes omgsr_quantize_mxfp8 makes of the bf16 form). A translation unit of its own, like gemm_mxfp8_out8.hip: the
// instantiations every other caller shares compile to what they were.
#include "gemm_mxfp8_body.hip.h"

namespace {
template <bool OUT8>
__global__ __launch_bounds__(512, 2) void mxfp8_gemm_geglu_kernel(const omgsr_igemm_args p, const IgemmGeo g, const IgemmOut8 o8) {
    // what mxfp8_gemm_geglu_ok pinned is written into a copy of the block as constants: the epilogue's run-time branches on them fold away
    // (the other activations, gate, residual, split and transposed outputs), and with them the scalar registers that kept them alive
    omgsr_igemm_args q = p;
    q.act = OMGSR_ACT_GEGLU;
    q.alpha = 1.0f;
    q.gate = nullptr; q.residual = nullptr; q.gn_partial = nullptr; q.overflow_flag = nullptr;
    q.res_el = OMGSR_EL_16; q.out_layout = OMGSR_LAYOUT_NHWC; q.out_lo_off = 0; q.out_mx = 0; q.batch = 1;
    if constexpr (OUT8) q.out_dtype = OMGSR_OUT_BF16;
    mxfp8_gemm_body<OUT8>(q, g, xcd_remap(blockIdx.x, g.ntm * g.ntn), 0, o8);
}
}  // namespace

namespace omgsr {
// What mxfp8_gemm_geglu_kernel runs (omgsr_igemm_geglu_mxfp8 refuses everything else with OMGSR_E_SHAPE). Cout counts logical columns (inner),
// Cout_pad the packed weight rows; the weight, its scales and the bias hold Cout_pad rows, so a tile past 2 x Cout reads the pack's zero rows
bool mxfp8_gemm_geglu_ok(const omgsr_igemm_args& a) {
    if (a.N <= 0 || a.H <= 0 || a.W <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.Ho <= 0 || a.Wo <= 0) return false;
    const int64_t M = (int64_t)a.N * a.Ho * a.Wo;
    return a.mxf8 == 1 && a.act == OMGSR_ACT_GEGLU && a.R == 1 && a.S == 1 && a.stride == 1 && a.pad_top == 0 && a.pad_left == 0 && a.upsample == 0 &&
           a.Ho == a.H && a.Wo == a.W && a.K_pad == a.Cin && (a.Cin % BK) == 0 && (a.in_ld == 0 || a.in_ld == a.Cin) && (a.Cout_pad % BN) == 0 &&
           (a.Cout % 32) == 0 && 2 * (int64_t)a.Cout <= a.Cout_pad && a.batch == 1 && a.out_layout == OMGSR_LAYOUT_NHWC && compute_dtype() == 0 &&
           (a.out_dtype == OMGSR_OUT_BF16 || a.out_dtype == OMGSR_OUT_F32) && !a.residual && !a.gate && !a.gn_partial && !a.gn_scale_shift &&
           !a.in_split && !a.w_split && a.mx_chunks16 == 0 && a.out_mx == 0 && a.out_lo_off == 0 && !a.weight_cm && !a.weight_ph && a.alpha == 1.0f &&
           a.in_scale && a.w_scale && a.out_ld >= 0 && (a.out_ld == 0 || a.out_ld >= a.Cout) && (a.out_ld & 7) == 0 && M < (1ll << 31) &&
           M * a.Cin < (1ll << 32) && (int64_t)a.Cout_pad * a.K_pad < (1ll << 32);
}

int mxfp8_gemm_geglu_launch(const omgsr_igemm_args& a, IgemmGeo g, unsigned char* out_scale, int64_t out_scale_ld, hipStream_t st, const double flops,
                            const double bytes) {
    g.ntm = (g.M + BM - 1) / BM;
    g.ntn = (2 * a.Cout + BN - 1) / BN;             // packed columns: <= Cout_pad / 256
    g.splits = 1;
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, g.M, 2 * a.Cout, (long long)a.Cin);
    if (ts.active) ts.rec.variant = 28;
    if (out_scale)
        return launch_lds<mxfp8_gemm_geglu_kernel<true>>(dim3(g.ntm * g.ntn, 1, 1), dim3(512), LDS_BYTES, st, a, g, IgemmOut8{out_scale, out_scale_ld});
    return launch_lds<mxfp8_gemm_geglu_kernel<false>>(dim3(g.ntm * g.ntn, 1, 1), dim3(512), LDS_BYTES, st, a, g, IgemmOut8{nullptr, 0});
}
}  // namespace omgsr
