// mxfp8_gemm_kernel's body (gemm_mxfp8_body.hip.h) as mxfp8_gemm_multi_kernel: up to 4 MXFP8 x MXFP8 token GEMMs in ONE launch
// (omgsr_igemm_mxfp8_multi, additive under ABI v22: no struct changes; timing variant 24). The fp8 tier's FLUX double blocks issue every
// projection twice, for the image tokens and for the text tokens; at small batches the text launch is a few dozen 256 x 256 tiles on 256 CUs
// and the image launch before it ends in a half-empty round, so the pair as one grid pays fewer rounds. The problems of a launch
// are independent: each has its own M, K, N, tensors, weight and epilogue; they share `batch` (grid.z), the compute type and this non-OUT8
// instantiation. A tile's bits do not depend on the launch it rides in: the body runs unchanged after the lookup, like
// igemm_halo_multi_kernel and mxfp8_conv_multi_kernel.
#include "gemm_mxfp8_body.hip.h"

namespace {

constexpr int MXG_MULTI_MAX = 4;
struct Mxfp8GemmMulti {
    omgsr_igemm_args p[MXG_MULTI_MAX];
    IgemmGeo g[MXG_MULTI_MAX];
    int start[MXG_MULTI_MAX + 1];
    int count;
};

// The workgroup looks its problem up in the prefix table of 8-aligned block ranges (wave-uniform: blockIdx and kernel arguments only), so
// xcd_remap of the local index keeps its meaning; a filler block of a range exits before any barrier. The body's M-groups of 8 row tiles
// work on the problem's own ntm / ntn.
__global__ __launch_bounds__(512, 2) void mxfp8_gemm_multi_kernel(const Mxfp8GemmMulti m) {
    int s = 0;
    while (s + 1 < m.count && (int)blockIdx.x >= m.start[s + 1]) ++s;
    const int bid = (int)blockIdx.x - m.start[s];
    const int ntiles = m.g[s].ntm * m.g[s].ntn;
    if (bid >= ntiles) return;
    mxfp8_gemm_body<false>(m.p[s], m.g[s], xcd_remap(bid, ntiles), blockIdx.z);
}

}  // namespace

namespace omgsr {
// `count` problems (2 ... 4) that omgsr_igemm_mxfp8_multi_ok accepted, in one launch; one timing entry with the summed work
int mxfp8_gemm_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, const int count, hipStream_t st, const double flops, const double bytes) {
    if (count < 2 || count > MXG_MULTI_MAX) return OMGSR_E_BADARG;
    Mxfp8GemmMulti m{};
    m.count = count;
    int at = 0;
    long long rows = 0;
    for (int i = 0; i < count; ++i) {
        if (a[i].batch != a[0].batch) return OMGSR_E_SHAPE;      // (omgsr_igemm_mxfp8_multi_ok refused it: never reached)
        m.p[i] = a[i];
        m.g[i] = g0[i];
        m.g[i].ntm = (m.g[i].M + BM - 1) / BM;
        m.g[i].ntn = (a[i].Cout + BN - 1) / BN;
        m.g[i].splits = 1;
        m.start[i] = at;
        at += (m.g[i].ntm * m.g[i].ntn + 7) & ~7;
        rows += (long long)m.g[i].M * a[i].batch;
    }
    for (int i = count; i <= MXG_MULTI_MAX; ++i) m.start[i] = at;
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, rows, a[0].Cout, (long long)a[0].Cin);
    if (ts.active) ts.rec.variant = 24;
    return launch_lds<mxfp8_gemm_multi_kernel>(dim3(at, 1, a[0].batch), dim3(512), LDS_BYTES, st, m);
}
}  // namespace omgsr
