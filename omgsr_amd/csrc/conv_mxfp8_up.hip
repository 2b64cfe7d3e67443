// MXFP8 x MXFP8 form of nearest-2x up-sampling + 3x3 stride-1 pad-1 convolution (the fp8 tier's opt-in VAE up-samplers; omgsr_conv_mxfp8_up,
// timing variant 25, kind 1; several problems of one layer in one launch: omgsr_conv_mxfp8_up_multi, mxfp8_conv_up_multi_kernel, variant 26 -
// the same tile body after the lookup).
//
// Both kernels are mxfp8_conv_tile<4, false> of conv_mxfp8_body.hip.h - read that header for the schedule, the lane map, the operand and
// weight layouts and the counted waits: the four-tap phase form (each of the four output phases is a 2 x 2 convolution of the LOW-resolution
// map with the phase-summed weights of ops.pack_conv_weight_mxfp8_up: fp64 sums, phase 2 a + b, tap 2 dy + dx), the patch's operand scale
// bytes (297 pixels x Cin / 32, at most 4864 bytes) resident in LDS behind the weight ring (78592 bytes in all: two workgroups per CU). The
// operand is omgsr_quantize_mxfp8 of the low-resolution stream tensor.
// Served (omgsr_conv_mxfp8_up_ok): the geometry for which the bf16 dispatcher picks the phase form, Cin % 128 == 0, Cin <= 512,
// Cout_pad % 128 == 0, bf16 compute type. The epilogue is the shared one (bias, act, gate, bf16 / fp32, stride-2 output rows, the four-phase
// GroupNorm statistic slots).
#include "conv_mxfp8_body.hip.h"
#include "timing.hip.h"

namespace {

using MXU = Mxfp8ConvTraits<4, false>;
constexpr int MXU_MAX_CIN = 512;
constexpr int MXU_SA_OFF = MXU::SA_OFF, MXU_SA_LD = 304;                         // operand scale bytes of the patch, [Cin / 32 blocks][patch row], rows padded 297 -> 304
constexpr int MXU_LDS_BYTES = MXU_SA_OFF + MXU_SA_LD * (MXU_MAX_CIN / 32);
static_assert(MXU_SA_LD == MXU::SA_LD && MXU_LDS_BYTES == MXU::lds_bytes(MXU_MAX_CIN), "the body's scale plane");
static_assert(MXU_LDS_BYTES <= 81920, "two workgroups per CU");

// Block orders: those of igemm_halo_kernel<TAPS = 4> (IgemmGeo.interleave; the chunked per-XCD order is the default). `tile` is the problem's
// logical tile index on the LOW-resolution grid, `phase` = 2 a + b.
__global__ __launch_bounds__(256, 2) void mxfp8_conv_up_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    int tile, phase;
    if (g.interleave) {
        if (!phase_block_map((int)blockIdx.x, g.ntm * g.ntn, 0, g.interleave == 2, tile, phase)) return;
    } else {
        tile = xcd_remap((int)blockIdx.x, g.ntm * g.ntn); phase = (int)blockIdx.y;
    }
    mxfp8_conv_tile<4, false>(p, g, tile, phase);
}

// Several problems that share the weight, its scales, Cin / Cout and the epilogue options in ONE launch (the tile-shape groups of a tiled-VAE
// layer; timing variant 26): HaloMulti as igemm_halo_multi_kernel<TAPS = 4> reads it - the workgroup looks its problem up in the prefix table
// of 8-aligned block ranges (wave-uniform: blockIdx and kernel arguments only), the filler blocks exit, and the same body runs unchanged.
__global__ __launch_bounds__(256, 2) void mxfp8_conv_up_multi_kernel(const HaloMulti m) {
    int s = 0, tile, phase;
    if (m.g[0].interleave) {
        while (s + 1 < m.count && (int)blockIdx.x >= 4 * m.start[s + 1]) ++s;
        if (!phase_block_map((int)blockIdx.x - 4 * m.start[s], m.g[s].ntm * m.g[s].ntn, m.start[s + 1] - m.start[s], m.g[0].interleave == 2, tile, phase)) return;
    } else {
        while (s + 1 < m.count && (int)blockIdx.x >= m.start[s + 1]) ++s;
        const int bid = (int)blockIdx.x - m.start[s];
        if (bid >= m.g[s].ntm * m.g[s].ntn) return;
        tile = xcd_remap(bid, m.g[s].ntm * m.g[s].ntn); phase = (int)blockIdx.y;
    }
    mxfp8_conv_tile<4, false>(m.p[s], m.g[s], tile, phase);
}

double up_bytes(const omgsr_igemm_args& a) {
    const double M = (double)a.N * a.Ho * a.Wo;
    return (1.0 + 1.0 / 32.0) * (double)a.N * a.H * a.W * a.Cin + M * a.Cout * (a.out_dtype == OMGSR_OUT_F32 ? 4.0 : 2.0);
}
double up_weight_bytes(const omgsr_igemm_args& a) { return (1.0 + 1.0 / 32.0) * 16.0 * (double)a.Cout_pad * a.Cin; }

}  // namespace

namespace omgsr {
// What mxfp8_conv_up_kernel itself needs (the dispatcher-side half of omgsr_conv_mxfp8_up_ok - "the bf16 path would take the phase form" -
// lives next to that dispatcher in igemm.hip)
bool mxfp8_conv_up_shape_ok(const omgsr_igemm_args& a) {
    return a.upsample == 1 && a.Ho == 2 * a.H && a.Wo == 2 * a.W && (a.Cin % 128) == 0 && a.Cin <= MXU_MAX_CIN && (a.Cout & 7) == 0 && !a.residual &&
           mxfp8_conv_common_shape_ok(a);
}

int mxfp8_conv_up_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const double flops) {
    if (halo_geo(a, g, true)) return OMGSR_E_SHAPE;           // (no narrow shape in the phase form: never reached)
    TimingScope ts(OMGSR_TK_IGEMM, flops, up_bytes(a) + up_weight_bytes(a), st, (long long)a.N * a.Ho * a.Wo, a.Cout, 9ll * a.Cin);
    if (ts.active) ts.rec.variant = 25;
    return launch_lds<mxfp8_conv_up_kernel>(halo_grid(g, true), dim3(256), MXU_LDS_BYTES, st, a, g);
}

// `count` problems (2 ... HALO_MULTI_MAX) that omgsr_conv_mxfp8_up_multi_ok accepted as one group, in one launch of mxfp8_conv_up_multi_kernel
int mxfp8_conv_up_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, const int count, hipStream_t st, const double flops) {
    if (count < 2 || count > HALO_MULTI_MAX) return OMGSR_E_BADARG;
    HaloMulti m{};
    const HaloPack k = halo_multi_pack(a, g0, count, true, m);
    if (k.narrow || k.flat) return OMGSR_E_SHAPE;             // (the phase form has neither: never reached)
    double M = 0.0, bytes = up_weight_bytes(a[0]);
    for (int i = 0; i < count; ++i) {
        M += (double)a[i].N * a[i].Ho * a[i].Wo;
        bytes += up_bytes(a[i]);
    }
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, (long long)M, a[0].Cout, 9ll * a[0].Cin);
    if (ts.active) ts.rec.variant = 26;
    return launch_lds<mxfp8_conv_up_multi_kernel>(halo_multi_grid(m.g[0], (unsigned)k.blocks, true), dim3(256), MXU_LDS_BYTES, st, m);
}
}  // namespace omgsr
