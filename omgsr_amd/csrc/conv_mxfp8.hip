// MXFP8 x MXFP8 3x3 stride-1 pad-1 convolution (the fp8 tier's opt-in VAE convs; omgsr_conv_mxfp8, timing variant 21, kind 1; several
// problems of one layer in one launch: omgsr_conv_mxfp8_multi, mxfp8_conv_multi_kernel, variant 22 - the same tile body after the lookup).
//
// mxfp8_conv_kernel runs the halo-tile schedule of igemm_halo_body.hip.h (8 x 32-pixel x 128-cout tile, patch LDS-DMA'd once per chunk and
// read by all nine taps at shifted rows, 3-deep weight ring, one raw barrier and one counted vmcnt wait per K-step, XCD remap) on fp8 codes:
//  * a chunk is 64 e4m3 channels = the same 64-byte patch rows and 8 KB weight slices as a 32-channel bf16 chunk, so patch geometry, DMA pieces
//    and the vmcnt arithmetic are the bf16 kernel's, while a K-step is one v_mfma_scale_f32_32x32x64_f8f6f4 per fragment pair (16 passes)
//    where bf16 issues two 32x32x16 of 8: the same matrix-pipe time for twice the contraction. One difference: patch rows are swizzled by
//    their patch COLUMN, not their row index (see a_ptr below) - 3 fragment address registers instead of 18, which is what fits the scale
//    registers into 256 VGPRs without spilling;
//  * operand: OMGSR_EL_MXFP8 as omgsr_quantize_mxfp8 / omgsr_groupnorm_apply_mxfp8 write it, rows = pixels: codes [N][H][W][Cin], scales
//    [N][H][W][Cin / 32];
//  * lane map (measured): lane l = (row l & 31, half h = l >> 5) holds K 16 h .. + 15 (registers 0-3) and 32 + 16 h .. + 15
//    (registers 4-7) of the 64, and the scale of hardware block b (K 32 b .. + 31 = the format's block 2 cc + b of chunk cc) is taken from lane
//    half b: a lane's two 16-byte reads are the patch row's 16-byte pieces h and 2 + h (as in the bf16 kernel), and it supplies the
//    E8M0 byte of block 2 cc + h of ITS row on both sides;
//  * operand scales: the whole patch's scale bytes (340 pixels x Cin / 32, at most 5504 bytes) are copied into LDS once per tile, behind the
//    weight ring (77184 bytes in all: two workgroups per CU), block-major so that a lane's byte of every (tap, fragment) is one per-chunk
//    base register plus an immediate; a lane reads one byte per fragment and K-step. Pixels outside the image read
//    the zero page (code 0) and a zero scale byte: exact zeros whatever the planes hold beyond the map;
//  * weight (ops.pack_conv_weight_mxfp8): one block per 32 consecutive input channels of one (cout, ky, kx), quantised by the format's rule.
//      codes  `weight_cm`: uint8 [Cin / 64][9 taps][Cout_pad][64]   (slice-major: a K-step's 128 x 64 slice is one contiguous 8 KB run)
//      scales `w_scale`:   uint8 [Cin / 64][Cout_pad][2 blocks][16] (byte t < 9 = tap t of that (chunk, cout, block); bytes 9-15 zero)
//    a lane fetches the 16 scale bytes of its two weight rows for a WHOLE chunk with two plain global loads (8 registers, single-buffered:
//    16 for a double buffer spill), issued in the last K-step of the previous chunk behind that step's MFMAs and in front of its weight
//    slice, so the counted wait of tap 0 (which leaves only that slice in flight) covers them; the tap's byte is shifted down with v_bfe. The loads are inline asm like the LDS-DMA pieces (a compiler-tracked load would make hipcc
//    insert vmcnt(0) at its first use and drain the prefetched patch), and their registers pass through an empty asm after the wait that
//    covers them so that no use can be scheduled in front of it.
// Served (omgsr_conv_mxfp8_ok): the geometry for which the bf16 dispatcher picks the spatial nine-tap form, Cin % 128 == 0, Cin <= 512,
// Cout_pad % 128 == 0, wide shape, bf16 compute type. The epilogue is the shared one (bias, act, gate, residual, bf16 / fp32, GroupNorm
// statistics).
#include "igemm_halo_body.hip.h"
#include "timing.hip.h"

namespace {

using MG = HaloGeo<9>;
constexpr int MXC_MAX_CIN = 512;
constexpr int MXC_SA_OFF = MG::LDS_BYTES, MXC_SA_LD = 344;                       // operand scale bytes of the patch, [Cin / 32 blocks][patch row], rows padded 340 -> 344
constexpr int MXC_LDS_BYTES = MXC_SA_OFF + MXC_SA_LD * (MXC_MAX_CIN / 32);
static_assert(MXC_SA_LD >= MG::PROWS, "scale plane pitch");
static_assert(MXC_LDS_BYTES <= 81920, "two workgroups per CU");

OMGSR_DEVINL u32x4_t gload16(const void* src) {
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}

// The tile body of both kernels below. `tile`: the problem's logical (XCD-remapped) tile index.
OMGSR_DEVINL void mxfp8_conv_body(const omgsr_igemm_args& p, const IgemmGeo& g, const int tile) {
    using T = bf16_t;
    constexpr int WTN = 64, FM = 4, FN = 2, BNK = 128, TAPS = 9;
    constexpr int PW = MG::PW, PROWS = MG::PROWS, APIECES = MG::APIECES, APW = MG::APW, A_BYTES = MG::A_BYTES;
    constexpr int NB = MG::NB, DUMMY_OFF = MG::DUMMY_OFF, B_OFF = MG::B_OFF;
    static_assert(APW == 6 && NB == 3, "the counted waits below");
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    const int tn = tile % g.ntn, tm = tile / g.ntn;
    const int per_img = g.tiles_x * g.tiles_y;
    const int img = tm / per_img;
    const int trem = tm - img * per_img;
    const int ty = trem / g.tiles_x, tx = trem - ty * g.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW, n0 = tn * BNK;

    const int Cin = p.Cin, nb = Cin >> 5, ncc = Cin >> 6;
    const unsigned char* __restrict__ in = reinterpret_cast<const unsigned char*>(p.in);
    const unsigned char* __restrict__ wt = reinterpret_cast<const unsigned char*>(p.weight_cm);
    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;

    const int lrow = lane >> 2;
    const int kc = (lane & 3) ^ ((lane >> 4) & 3);           // weight slices: source piece for LDS position (lane & 3), swizzled by the row as in halo_body

    // patch pieces: piece j = wave * 6 + i covers patch rows [16 j, 16 j + 16); patch row -> (py, px)
    const unsigned char* a_ptr[APW];
    unsigned a_ok = 0;                                       // bit i: piece i of this lane lies in the image (its pointer advances 64 bytes per chunk)
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int pr = 16 * (wave * APW + i) + lrow;
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + py, vx = x0 - 1 + px;
        const bool ok = (wave * APW + i) < APIECES && pr < PROWS && (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
        // patch rows are swizzled by their patch COLUMN ((px >> 2) & 3) where halo_body swizzles by the patch row index: 16 consecutive pixels of a
        // tile row still hit 16 distinct 16-byte slots, and a fragment's address becomes (tile row) x pitch + f(column) - the tile-row term an
        // immediate of the ds_read, so 3 address registers (one per kx) serve the 36 (tap, fragment) pairs instead of 18
        const int kca = (lane & 3) ^ ((px >> 2) & 3);
        a_ptr[i] = ok ? in + pix * Cin + kca * 16 : reinterpret_cast<const unsigned char*>(g_zero_page_h);
        a_ok |= (ok ? 1u : 0u) << i;
    }
    const unsigned char* b_ptr[BPW];
#pragma unroll
    for (int i = 0; i < BPW; ++i) b_ptr[i] = wt + (int64_t)(n0 + 16 * (wave * BPW + i) + lrow) * 64 + kc * 16;
    const int64_t b_step = (int64_t)p.Cout_pad * 64;       // bytes between consecutive (chunk, tap) slices

    auto issue_a = [&](const int buf) {
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int piece = wave * APW + i;
            const unsigned dst = piece < APIECES ? lds_base + buf * A_BYTES + piece * 1024 : lds_base + DUMMY_OFF + (piece - APIECES) * 1024;
            glds16(a_ptr[i], __builtin_amdgcn_readfirstlane(dst));
            a_ptr[i] += ((a_ok >> i) & 1u) << 6;
        }
    };
    auto issue_b = [&](const int stage) {
        const unsigned dst = lds_base + B_OFF + stage * B_BYTES + (wave * BPW) * 1024;
#pragma unroll
        for (int i = 0; i < BPW; ++i) {
            glds16(b_ptr[i], __builtin_amdgcn_readfirstlane(dst + i * 1024));
            b_ptr[i] += b_step;
        }
    };

    const int frow = lane & 31;
    const int half = lane >> 5;
    // weight scales of the lane's two rows (cout n0 + 64 wn + 32 j + frow, block `half`), one 16-byte group per chunk
    const unsigned char* ws_ptr = p.w_scale + ((int64_t)(n0 + wn * WTN + frow) * 2 + half) * 16;
    const int64_t ws_step = (int64_t)p.Cout_pad * 32;
    u32x4_t ws[FN];
    auto issue_ws = [&]() {
#pragma unroll
        for (int j = 0; j < FN; ++j) ws[j] = gload16(ws_ptr + j * (32 * 32));
        ws_ptr += ws_step;
    };

    f32x16_t acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int nsteps = ncc * TAPS;
    const int bsw = (frow >> 2) & 3;
    const int boff0 = (wn * WTN) * 64 + frow * 64 + ((half) ^ bsw) * 16;
    const int boff1 = (wn * WTN) * 64 + frow * 64 + ((2 + half) ^ bsw) * 16;
    // fragment i of tap (ky, kx): patch row (4 wm + i + ky) PW + frow + kx = aoff[kx] + (i + ky) PW 64 (an immediate; a multiple of 128, so it
    // commutes with the ^ 32 that selects the lane's second 16-byte piece)
    int aoff[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) aoff[kx] = (FM * wm * PW + frow + kx) * 64 + ((half ^ (((frow + kx) >> 2) & 3)) << 4);
    static_assert((PW * 64) % 128 == 0 && A_BYTES % 128 == 0, "immediates must not touch bit 5");

    issue_ws();
    issue_a(0);
    issue_b(0);
    issue_b(1);

    // the patch's operand scales -> LDS (ordinary loads and ds_writes: the compiler waits for them; the first K-step's barrier publishes them)
    for (int pr = t; pr < PROWS; pr += 256) {
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + py, vx = x0 - 1 + px;
        const bool ok = (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
        const unsigned* src = reinterpret_cast<const unsigned*>(p.in_scale + pix * nb);
        unsigned char* dst = lds + MXC_SA_OFF + pr;
        for (int q = 0; q < (nb >> 2); ++q) {
            const unsigned w = ok ? src[q] : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(4 * q + e) * MXC_SA_LD] = (unsigned char)(w >> (8 * e));
        }
    }
    // a lane's scale byte of fragment i, tap (ky, kx), chunk cc: block 2 cc + half of patch row (4 wm + i + ky) PW + frow + kx
    const int sa_base = MXC_SA_OFF + half * MXC_SA_LD + FM * wm * PW + frow;

    // one K-step with compile-time tap and patch parity (see halo_body for the wait / barrier / late-issue reasoning, unchanged here)
    auto step = [&](auto tap_c, auto par_c, const int cc, const int s) {
        constexpr int tap = decltype(tap_c)::value, par = decltype(par_c)::value;
        if constexpr (tap == 1) {
            if (cc + 1 < ncc) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        } else if constexpr (tap == TAPS - 1) {
            if (s + 1 < nsteps) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (tap == 0) {
            // this chunk's weight scales were issued in the previous step (or the prologue) in front of its weight slice: the wait above,
            // which leaves only that slice in flight, covers them
#pragma unroll
            for (int j = 0; j < FN; ++j) asm volatile("" : "+v"(ws[j]));
        }
        auto issue_dma = [&]() {
            if constexpr (tap == 0) { if (cc + 1 < ncc) issue_a(par ^ 1); }
            if constexpr (tap == TAPS - 1) { if (cc + 1 < ncc) issue_ws(); }        // (this step's own bytes were extracted above)
            if (s + 2 < nsteps) issue_b((tap + 2) % NB);
        };

        const unsigned char* As = lds + par * A_BYTES;
        const unsigned char* Bs = lds + B_OFF + (tap % NB) * B_BYTES;
        const unsigned char* Ss = lds + sa_base + (2 * cc) * MXC_SA_LD;
        i32x8_t a8[FM], b8[FN];
        int sa[FM], sb[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            a8[i] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(As + (i + tap / 3) * PW * 64 + aoff[tap % 3]),
                                            *reinterpret_cast<const i32x4_t*>(As + (i + tap / 3) * PW * 64 + (aoff[tap % 3] ^ 32)), 0, 1, 2, 3, 4, 5, 6, 7);
            sa[i] = Ss[(i + tap / 3) * PW + tap % 3];           // (an immediate offset of the ds_read: no address arithmetic in the loop)
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            b8[j] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff0), *reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff1),
                                            0, 1, 2, 3, 4, 5, 6, 7);
            sb[j] = (int)__builtin_amdgcn_ubfe(ws[j][tap >> 2], (unsigned)(8 * (tap & 3)), 8u);
        }
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
            for (int j = 0; j < FN; ++j)
                // inline asm keeps the tied accumulators in place; s_nop 3: hipcc pads no hazards around inline asm and the scale operands
                // are VALU / LDS results (igemm_halo_body.hip.h has the history)
                asm volatile("s_nop 3\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                             : "+v"(acc[i][j]) : "v"(b8[j]), "v"(a8[i]), "v"(sb[j]), "v"(sa[i]));   // transposed tile
            if (i == FM / 2 - 1) {
                __builtin_amdgcn_sched_barrier(0);
                issue_dma();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    auto chunk = [&](auto par_c, const int cc) {
        const int s0 = cc * TAPS;
        step(std::integral_constant<int, 0>{}, par_c, cc, s0 + 0);
        step(std::integral_constant<int, 1>{}, par_c, cc, s0 + 1);
        step(std::integral_constant<int, 2>{}, par_c, cc, s0 + 2);
        step(std::integral_constant<int, 3>{}, par_c, cc, s0 + 3);
        step(std::integral_constant<int, 4>{}, par_c, cc, s0 + 4);
        step(std::integral_constant<int, 5>{}, par_c, cc, s0 + 5);
        step(std::integral_constant<int, 6>{}, par_c, cc, s0 + 6);
        step(std::integral_constant<int, 7>{}, par_c, cc, s0 + 7);
        step(std::integral_constant<int, 8>{}, par_c, cc, s0 + 8);
    };
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");        // (the asm MFMAs below are invisible to the compiler's hazard padding)
    for (int cc = 0; cc < ncc; cc += 2) {
        chunk(std::integral_constant<int, 0>{}, cc);
        if (cc + 1 < ncc) chunk(std::integral_constant<int, 1>{}, cc + 1);
    }
    // the last asm MFMAs (16 passes each) must have written the accumulators before the epilogue's VALU reads them
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");

    int mb[FM], nv[FM];
    int colsv = p.Wo - x0; colsv = colsv > TW ? TW : colsv;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int y = y0 + FM * wm + i;
        mb[i] = (img * p.Ho + y) * p.Wo + x0;
        nv[i] = (y < p.Ho) ? colsv : 0;
    }
    float* epi = reinterpret_cast<float*>(lds) + wave * 32 * (WTN + 4);
    // fused GroupNorm statistics: slot = (spatial tile, upper / lower 4 tile rows), [N][2 * tiles][G][2] - the bf16 halo kernel's layout
    const int64_t slot = (int64_t)(img * per_img + trem) * 2 + wm;
    float* gn_dst = p.gn_partial ? p.gn_partial + slot * p.gn_entries * 2 : nullptr;
    igemm_epilogue<T, WTN, FM, FN>(p, acc, epi, lane, mb, nv, n0 + wn * WTN, 0, gn_dst, 0, 1, 0);
}

__global__ __launch_bounds__(256, 2) void mxfp8_conv_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    mxfp8_conv_body(p, g, xcd_remap((int)blockIdx.x, g.ntm * g.ntn));
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
    mxfp8_conv_body(m.p[s], m.g[s], xcd_remap(bid, ntiles));
}

}  // namespace

namespace omgsr {
// What mxfp8_conv_kernel itself needs (the dispatcher-side half of omgsr_conv_mxfp8_ok - "the bf16 path would take the spatial nine-tap
// form" - lives next to that dispatcher in igemm.hip)
bool mxfp8_conv_shape_ok(const omgsr_igemm_args& a) {
    return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad_top == 1 && a.pad_left == 1 && a.upsample == 0 && a.Ho == a.H && a.Wo == a.W &&
           (a.Cin % 128) == 0 && a.Cin <= MXC_MAX_CIN && a.K_pad == 9 * a.Cin && (a.in_ld == 0 || a.in_ld == a.Cin) && (a.Cout_pad % BN) == 0 &&
           a.Cout >= 96 && a.act != OMGSR_ACT_GEGLU && a.out_layout == OMGSR_LAYOUT_NHWC && a.batch == 1 && !a.in_split && !a.w_split &&
           a.mx_chunks16 == 0 && a.out_mx == 0 && a.out_lo_off == 0 && !a.gn_scale_shift && !a.weight_ph && a.mxf8 == 0 && compute_dtype() == 0;
}

int mxfp8_conv_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const double flops) {
    const bool narrow = halo_geo(a, g, false);
    if (narrow || g.flat) return OMGSR_E_SHAPE;               // (omgsr_conv_mxfp8_ok refused both: never reached)
    const double M = (double)a.N * a.Ho * a.Wo;
    const double bytes = (1.0 + 1.0 / 32.0) * ((double)a.N * a.H * a.W * a.Cin + (double)a.Cout_pad * a.K_pad) +
                         M * a.Cout * ((a.out_dtype == OMGSR_OUT_F32 ? 4.0 : 2.0) + (a.residual ? (a.res_el == OMGSR_EL_F32 ? 4.0 : 2.0) : 0.0));
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, (long long)M, a.Cout, 9ll * a.Cin);
    if (ts.active) ts.rec.variant = 21;
    return launch_lds<mxfp8_conv_kernel>(dim3(g.ntm * g.ntn), dim3(256), MXC_LDS_BYTES, st, a, g);
}

// `count` problems (2 ... HALO_MULTI_MAX) that omgsr_conv_mxfp8_multi_ok accepted as one group, in one launch of mxfp8_conv_multi_kernel
int mxfp8_conv_launch_multi(const omgsr_igemm_args* a, const IgemmGeo* g0, const int count, hipStream_t st, const double flops) {
    if (count < 2 || count > HALO_MULTI_MAX) return OMGSR_E_BADARG;
    HaloMulti m{};
    const HaloPack k = halo_multi_pack(a, g0, count, false, m);
    if (k.narrow || k.flat) return OMGSR_E_SHAPE;             // (omgsr_conv_mxfp8_multi_ok refused both: never reached)
    double M = 0.0, bytes = (1.0 + 1.0 / 32.0) * (double)a[0].Cout_pad * a[0].K_pad;
    for (int i = 0; i < count; ++i) {
        const double Mi = (double)a[i].N * a[i].Ho * a[i].Wo;
        M += Mi;
        bytes += (1.0 + 1.0 / 32.0) * (double)a[i].N * a[i].H * a[i].W * a[i].Cin +
                 Mi * a[i].Cout * ((a[i].out_dtype == OMGSR_OUT_F32 ? 4.0 : 2.0) + (a[i].residual ? (a[i].res_el == OMGSR_EL_F32 ? 4.0 : 2.0) : 0.0));
    }
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, (long long)M, a[0].Cout, 9ll * a[0].Cin);
    if (ts.active) ts.rec.variant = 22;
    return launch_lds<mxfp8_conv_multi_kernel>(dim3(k.blocks), dim3(256), MXC_LDS_BYTES, st, m);
}
}  // namespace omgsr
