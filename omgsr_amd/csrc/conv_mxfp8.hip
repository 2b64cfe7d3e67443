// MXFP8 x MXFP8 3x3 stride-1 pad-1 convolution (the fp8 tier's opt-in VAE convs; omgsr_conv_mxfp8, timing variant 21, kind 1; several
// problems of one layer in one launch: omgsr_conv_mxfp8_multi, mxfp8_conv_multi_kernel, variant 22 - the same tile body after the lookup).
//
// Both kernels are mxfp8_conv_tile<9, false> of conv_mxfp8_body.hip.h - read that header for the schedule, the lane map, the operand and
// weight layouts and the counted waits: nine taps, the whole patch's operand scale bytes (340 pixels x Cin / 32, at most 5504 bytes) resident
// in LDS behind the weight ring (77184 bytes in all: two workgroups per CU).
// Served (omgsr_conv_mxfp8_ok): the geometry for which the bf16 dispatcher picks the spatial nine-tap form, Cin % 128 == 0, Cin <= 512,
// Cout_pad % 128 == 0, wide shape, bf16 compute type. The epilogue is the shared one (bias, act, gate, residual, bf16 / fp32, GroupNorm
// statistics).
#include "conv_mxfp8_body.hip.h"
#include "timing.hip.h"

namespace {

using MXC = Mxfp8ConvTraits<9, false>;
constexpr int MXC_MAX_CIN = 512;
constexpr int MXC_SA_OFF = MXC::SA_OFF, MXC_SA_LD = 344;                         // operand scale bytes of the patch, [Cin / 32 blocks][patch row], rows padded 340 -> 344
constexpr int MXC_LDS_BYTES = MXC_SA_OFF + MXC_SA_LD * (MXC_MAX_CIN / 32);
static_assert(MXC_SA_LD == MXC::SA_LD && MXC_LDS_BYTES == MXC::lds_bytes(MXC_MAX_CIN), "the body's scale plane");
static_assert(MXC_LDS_BYTES <= 81920, "two workgroups per CU");

// Both kernels hand the body the problem's logical (XCD-remapped) tile index; the nine-tap forms have no phase.
__global__ __launch_bounds__(256, 2) void mxfp8_conv_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    mxfp8_conv_tile<9, false>(p, g, xcd_remap((int)blockIdx.x, g.ntm * g.ntn), 0);
}

// Several problems that share the weight, its scales, Cin / Cout and the epilogue options in ONE launch (the tile-shape groups of a tiled-VAE
// layer; timing variant 22): HaloMulti as igemm_halo_multi_kernel reads it - the workgroup looks its problem up in the prefix table of
// 8-aligned block ranges (wave-uniform: blockIdx and kernel arguments only), the filler blocks exit, and the body above runs unchanged.
__global__ __launch_bounds__(256, 2) void mxfp8_conv_multi_kernel(const HaloMulti m) {
    int s = 0;
    while (s + 1 < m.count && (int)blockIdx.x >= m.start[s + 1]) ++s;
    const int bid = (int)blockIdx.x - m.start[s];
    const int ntiles = m.g[s].ntm * m.g[s].ntn;
    if (bid >= ntiles) return;
    mxfp8_conv_tile<9, false>(m.p[s], m.g[s], xcd_remap(bid, ntiles), 0);
}

}  // namespace

namespace omgsr {
// What mxfp8_conv_kernel itself needs (the dispatcher-side half of omgsr_conv_mxfp8_ok - "the bf16 path would take the spatial nine-tap
// form" - lives next to that dispatcher in igemm.hip)
bool mxfp8_conv_shape_ok(const omgsr_igemm_args& a) {
    return a.upsample == 0 && a.Ho == a.H && a.Wo == a.W && (a.Cin % 128) == 0 && a.Cin <= MXC_MAX_CIN && !a.weight_ph && mxfp8_conv_common_shape_ok(a);
}

int mxfp8_conv_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const double flops) {
    const bool narrow = halo_geo(a, g, false);
    if (narrow || g.flat) return OMGSR_E_SHAPE;               // (omgsr_conv_mxfp8_ok refused both: never reached)
    TimingScope ts(OMGSR_TK_IGEMM, flops, conv9_bytes(a) + conv9_weight_bytes(a), st, (long long)a.N * a.Ho * a.Wo, a.Cout, 9ll * a.Cin);
    if (ts.active) ts.rec.variant = 21;
    return launch_lds<mxfp8_conv_kernel>(dim3(g.ntm * g.ntn), dim3(256), MXC_LDS_BYTES, st, a, g);
}

// `count` problems (2 ... HALO_MULTI_MAX) that omgsr_conv_mxfp8_multi_ok accepted as one group, in one launch of mxfp8_conv_multi_kernel
int mxfp8_conv_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, const int count, hipStream_t st, const double flops) {
    if (count < 2 || count > HALO_MULTI_MAX) return OMGSR_E_BADARG;
    HaloMulti m{};
    const HaloPack k = halo_multi_pack(a, g0, count, false, m);
    if (k.narrow || k.flat) return OMGSR_E_SHAPE;             // (omgsr_conv_mxfp8_multi_ok refused both: never reached)
    double M = 0.0, bytes = conv9_weight_bytes(a[0]);
    for (int i = 0; i < count; ++i) {
        M += (double)a[i].N * a[i].Ho * a[i].Wo;
        bytes += conv9_bytes(a[i]);
    }
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, (long long)M, a[0].Cout, 9ll * a[0].Cin);
    if (ts.active) ts.rec.variant = 22;
    return launch_lds<mxfp8_conv_multi_kernel>(dim3(k.blocks), dim3(256), MXC_LDS_BYTES, st, m);
}
}  // namespace omgsr
