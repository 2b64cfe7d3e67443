// Deep-K form of the MXFP8 x MXFP8 3x3 stride-1 pad-1 convolution (OMGSR-S's opt-in UNet resnet convs on the bf16 tier; omgsr_conv_mxfp8_deep,
// timing variant 27, kind 1).
//
// mxfp8_conv_deep_kernel is mxfp8_conv_tile<9, true> of conv_mxfp8_body.hip.h - read that header for the schedule, the lane map, the operand
// and weight layouts, the counted waits and the refill timeline: conv_mxfp8.hip's nine-tap body with the operand SCALE plane windowed instead
// of resident, which lifts that kernel's two limits:
//  * Cin % 64 == 0 (not % 128): nothing wider than one chunk's 2-byte scale pair of a pixel is ever read;
//  * Cin up to 2048 (not 512): the LDS holds the scale bytes of a WINDOW of MXD_WINDOW_CHUNKS = 1 chunk (2 blocks x 344-byte rows = 688 bytes),
//    double-buffered: 71680 + 2 x 688 = 73056 bytes whatever Cin is (two workgroups per CU).
// Served (omgsr_conv_mxfp8_deep_ok): omgsr_conv_mxfp8_ok's rules with Cin % 64 == 0, Cin <= 2048. The epilogue is the shared one.
#include "conv_mxfp8_body.hip.h"
#include "timing.hip.h"

namespace {

using MXD = Mxfp8ConvTraits<9, true>;
constexpr int MXD_MAX_CIN = 2048;
constexpr int MXD_WINDOW_CHUNKS = 1;                                             // chunks of operand scales per LDS window (see the shared header)
constexpr int MXD_SA_OFF = MXD::SA_OFF, MXD_SA_LD = 344;                         // a window: [2 blocks][patch row], rows padded 340 -> 344
constexpr int MXD_WIN_BYTES = MXD_WINDOW_CHUNKS * 2 * MXD_SA_LD;
constexpr int MXD_LDS_BYTES = MXD_SA_OFF + 2 * MXD_WIN_BYTES;                    // double-buffered
static_assert(MXD_WINDOW_CHUNKS == MXD::WINDOW_CHUNKS && MXD_SA_LD == MXD::SA_LD && MXD_LDS_BYTES == MXD::lds_bytes(MXD_MAX_CIN), "the body's scale window");
static_assert(MXD_LDS_BYTES <= 81920, "two workgroups per CU");

// `tile`: the problem's logical (XCD-remapped) tile index.
__global__ __launch_bounds__(256, 2) void mxfp8_conv_deep_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    mxfp8_conv_tile<9, true>(p, g, xcd_remap((int)blockIdx.x, g.ntm * g.ntn), 0);
}

}  // namespace

namespace omgsr {
// What mxfp8_conv_deep_kernel itself needs (the dispatcher-side half of omgsr_conv_mxfp8_deep_ok - "the bf16 path would take the spatial
// nine-tap form" - lives next to that dispatcher in igemm.hip): mxfp8_conv_shape_ok's rules with the two Cin limits replaced
bool mxfp8_conv_deep_shape_ok(const omgsr_igemm_args& a) {
    return a.upsample == 0 && a.Ho == a.H && a.Wo == a.W && (a.Cin % 64) == 0 && a.Cin > 0 && a.Cin <= MXD_MAX_CIN && !a.weight_ph && mxfp8_conv_common_shape_ok(a);
}

int mxfp8_conv_deep_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const double flops) {
    const bool narrow = halo_geo(a, g, false);
    if (narrow || g.flat) return OMGSR_E_SHAPE;               // (omgsr_conv_mxfp8_deep_ok refused both: never reached)
    TimingScope ts(OMGSR_TK_IGEMM, flops, conv9_bytes(a) + conv9_weight_bytes(a), st, (long long)a.N * a.Ho * a.Wo, a.Cout, 9ll * a.Cin);
    if (ts.active) ts.rec.variant = 27;
    return launch_lds<mxfp8_conv_deep_kernel>(dim3(g.ntm * g.ntn), dim3(256), MXD_LDS_BYTES, st, a, g);
}
}  // namespace omgsr
