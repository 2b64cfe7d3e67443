// MXFP8 x MXFP8 form of nearest-2x up-sampling + 3x3 stride-1 pad-1 convolution (the fp8 tier's opt-in VAE up-samplers; omgsr_conv_mxfp8_up,
// timing variant 25, kind 1; several problems of one layer in one launch: omgsr_conv_mxfp8_up_multi, mxfp8_conv_up_multi_kernel, variant 26 -
// the same tile body after the lookup).
//
// mxfp8_conv_up_kernel is the phase form of igemm_halo_body.hip.h (HaloGeo<4>: output pixel (2y + a, 2x + b) only sees the 2 x 2 low-resolution
// pixels rows {y - 1 + a, y + a} x columns {x - 1 + b, x + b}, so each of the four phases is a 2 x 2 convolution of the LOW-resolution map with
// phase-summed weights; 8 x 32 low-resolution-pixel x 128-cout tile, 9 x 33 = 297-row patch LDS-DMA'd once per chunk in 19 pieces, 5 per
// wave, 4-deep weight ring with stage = tap, one raw barrier and one counted vmcnt wait per K-step, chunked per-XCD phase order) run on fp8
// codes the way mxfp8_conv_body (conv_mxfp8.hip) runs the nine-tap form:
//  * a chunk is 64 e4m3 channels = the same 64-byte patch rows and 8 KB weight slices as a 32-channel bf16 chunk; a K-step is one
//    v_mfma_scale_f32_32x32x64_f8f6f4 per fragment pair (with the s_nop padding every scaled MFMA of this library carries); patch rows are
//    swizzled by their patch COLUMN, so 2 fragment address registers (one per tap column) serve the 16 (tap, fragment) pairs;
//  * operand: OMGSR_EL_MXFP8 as omgsr_quantize_mxfp8 writes it from the low-resolution stream tensor, rows = pixels: codes [N][H][W][Cin],
//    scales [N][H][W][Cin / 32];
//  * lane map (measured): lane l = (row l & 31, half h = l >> 5) holds K 16 h .. + 15 (registers 0-3) and 32 + 16 h .. + 15
//    (registers 4-7) of the 64 and supplies the E8M0 byte of block 2 cc + h of ITS row on both sides;
//  * operand scales: the patch's scale bytes (297 pixels x Cin / 32, at most 4864 bytes) are copied into LDS once per tile, behind the
//    weight ring (78592 bytes in all: two workgroups per CU), block-major: a lane's byte of every (tap, fragment) is one per-chunk base
//    plus an immediate. Pixels outside the low-resolution map read the zero page (code 0) and a zero scale byte: exact zeros;
//  * weight (ops.pack_conv_weight_mxfp8_up): the four phase-summed 2 x 2 kernels (fp64 sums, phase 2 a + b, tap 2 dy + dx), one block per 32
//    consecutive input channels of one (phase, cout, tap), quantised by the format's rule.
//      codes  `weight_ph`: uint8 [4 phases][Cin / 64][4 taps][Cout_pad][64]   (slice-major: a K-step's 128 x 64 slice is one 8 KB run)
//      scales `w_scale`:   uint8 [4 phases][Cin / 64][Cout_pad][2 blocks][4 taps]
//    a lane fetches the 4 scale bytes of each of its two weight rows for a WHOLE chunk with one inline-asm dword load per row (2 registers,
//    single-buffered), issued in the last K-step of the previous chunk in front of that step's weight slice, so the counted wait of tap 0
//    (which leaves only that slice in flight) covers them; the tap's byte is shifted down with v_bfe.
// Served (omgsr_conv_mxfp8_up_ok): the geometry for which the bf16 dispatcher picks the phase form, Cin % 128 == 0, Cin <= 512,
// Cout_pad % 128 == 0, bf16 compute type. The epilogue is the shared one (bias, act, gate, bf16 / fp32, stride-2 output rows, the four-phase
// GroupNorm statistic slots).
#include "igemm_halo_body.hip.h"
#include "timing.hip.h"

namespace {

using UG = HaloGeo<4>;
constexpr int MXU_MAX_CIN = 512;
constexpr int MXU_SA_OFF = UG::LDS_BYTES, MXU_SA_LD = 304;                       // operand scale bytes of the patch, [Cin / 32 blocks][patch row], rows padded 297 -> 304
constexpr int MXU_LDS_BYTES = MXU_SA_OFF + MXU_SA_LD * (MXU_MAX_CIN / 32);
static_assert(MXU_SA_LD >= UG::PROWS, "scale plane pitch");
static_assert(MXU_LDS_BYTES <= 81920, "two workgroups per CU");

OMGSR_DEVINL unsigned gload4(const void* src) {
    unsigned v;
    asm volatile("global_load_dword %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}

// The tile body of both kernels below. `tile`: the problem's logical tile index on the LOW-resolution grid, `phase` = 2 a + b.
OMGSR_DEVINL void mxfp8_conv_up_body(const omgsr_igemm_args& p, const IgemmGeo& g, const int tile, const int phase) {
    using T = bf16_t;
    constexpr int WTN = 64, FM = 4, FN = 2, BNK = 128, TAPS = 4;
    constexpr int PW = UG::PW, PROWS = UG::PROWS, APIECES = UG::APIECES, APW = UG::APW, A_BYTES = UG::A_BYTES;
    constexpr int NB = UG::NB, DUMMY_OFF = UG::DUMMY_OFF, B_OFF = UG::B_OFF;
    static_assert(APW == 5 && NB == 4 && PW == 33, "the counted waits below");
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int ph_a = phase >> 1, ph_b = phase & 1;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    const int tn = tile % g.ntn, tm = tile / g.ntn;
    const int per_img = g.tiles_x * g.tiles_y;
    const int img = tm / per_img;
    const int trem = tm - img * per_img;
    const int ty = trem / g.tiles_x, tx = trem - ty * g.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW, n0 = tn * BNK;          // (low-resolution coordinates)

    const int Cin = p.Cin, nb = Cin >> 5, ncc = Cin >> 6;
    const unsigned char* __restrict__ in = reinterpret_cast<const unsigned char*>(p.in);
    const unsigned char* __restrict__ wt = reinterpret_cast<const unsigned char*>(p.weight_ph) + (int64_t)phase * ncc * TAPS * p.Cout_pad * 64;
    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;

    const int lrow = lane >> 2;
    const int kc = (lane & 3) ^ ((lane >> 4) & 3);           // weight slices: source piece for LDS position (lane & 3), swizzled by the row as in halo_body

    // patch pieces: piece j = wave * 5 + i covers patch rows [16 j, 16 j + 16); patch row -> (py, px); phase (a, b) reads low-resolution rows
    // y - 1 + a, y + a (columns likewise)
    const unsigned char* a_ptr[APW];
    unsigned a_ok = 0;                                       // bit i: piece i of this lane lies in the map (its pointer advances 64 bytes per chunk)
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int pr = 16 * (wave * APW + i) + lrow;
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + ph_a + py, vx = x0 - 1 + ph_b + px;
        const bool ok = (wave * APW + i) < APIECES && pr < PROWS && (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
        const int kca = (lane & 3) ^ ((px >> 2) & 3);          // swizzled by the patch COLUMN (see mxfp8_conv_body)
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
    // weight scales of the lane's two rows (cout n0 + 64 wn + 32 j + frow, block `half`), one dword (4 taps) per chunk
    const unsigned char* ws_ptr = p.w_scale + (int64_t)phase * ncc * p.Cout_pad * 8 + ((int64_t)(n0 + wn * WTN + frow) * 2 + half) * 4;
    const int64_t ws_step = (int64_t)p.Cout_pad * 8;
    unsigned ws[FN];
    auto issue_ws = [&]() {
#pragma unroll
        for (int j = 0; j < FN; ++j) ws[j] = gload4(ws_ptr + j * (32 * 8));
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
    // fragment i of tap (dy, dx): patch row (4 wm + i + dy) PW + frow + dx = aoff[dx] + (i + dy) PW 64 (an immediate; a multiple of 64, so it
    // leaves the 16-byte slot bits - the swizzle and the ^ 32 that selects the lane's second piece - alone)
    int aoff[2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) aoff[dx] = (FM * wm * PW + frow + dx) * 64 + ((half ^ (((frow + dx) >> 2) & 3)) << 4);

    issue_ws();
    issue_a(0);
    issue_b(0);
    issue_b(1);

    // the patch's operand scales -> LDS (ordinary loads and ds_writes: the compiler waits for them; the first K-step's barrier publishes them)
    for (int pr = t; pr < PROWS; pr += 256) {
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + ph_a + py, vx = x0 - 1 + ph_b + px;
        const bool ok = (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
        const unsigned* src = reinterpret_cast<const unsigned*>(p.in_scale + pix * nb);
        unsigned char* dst = lds + MXU_SA_OFF + pr;
        for (int q = 0; q < (nb >> 2); ++q) {
            const unsigned w = ok ? src[q] : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(4 * q + e) * MXU_SA_LD] = (unsigned char)(w >> (8 * e));
        }
    }
    // a lane's scale byte of fragment i, tap (dy, dx), chunk cc: block 2 cc + half of patch row (4 wm + i + dy) PW + frow + dx
    const int sa_base = MXU_SA_OFF + half * MXU_SA_LD + FM * wm * PW + frow;

    // one K-step with compile-time tap and patch parity (see halo_body for the wait / barrier / late-issue reasoning, unchanged here)
    auto step = [&](auto tap_c, auto par_c, const int cc, const int s) {
        constexpr int tap = decltype(tap_c)::value, par = decltype(par_c)::value;
        if constexpr (tap == 1) {
            // the previous step (tap 0) issued the next chunk's patch (5 pieces) and one weight slice (2)
            if (cc + 1 < ncc) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory");
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

        constexpr int dy = tap >> 1, dx = tap & 1;
        const unsigned char* As = lds + par * A_BYTES;
        const unsigned char* Bs = lds + B_OFF + tap * B_BYTES;
        const unsigned char* Ss = lds + sa_base + (2 * cc) * MXU_SA_LD;
        i32x8_t a8[FM], b8[FN];
        int sa[FM], sb[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            a8[i] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(As + (i + dy) * PW * 64 + aoff[dx]),
                                            *reinterpret_cast<const i32x4_t*>(As + (i + dy) * PW * 64 + (aoff[dx] ^ 32)), 0, 1, 2, 3, 4, 5, 6, 7);
            sa[i] = Ss[(i + dy) * PW + dx];                     // (an immediate offset of the ds_read: no address arithmetic in the loop)
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            b8[j] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff0), *reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff1),
                                            0, 1, 2, 3, 4, 5, 6, 7);
            sb[j] = (int)__builtin_amdgcn_ubfe(ws[j], (unsigned)(8 * tap), 8u);
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
    };
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");        // (the asm MFMAs below are invisible to the compiler's hazard padding)
    for (int cc = 0; cc < ncc; cc += 2) {
        chunk(std::integral_constant<int, 0>{}, cc);
        if (cc + 1 < ncc) chunk(std::integral_constant<int, 1>{}, cc + 1);
    }
    // the last asm MFMAs (16 passes each) must have written the accumulators before the epilogue's VALU reads them
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");

    int mb[FM], nv[FM];
    int colsv = p.W - x0; colsv = colsv > TW ? TW : colsv;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int y = y0 + FM * wm + i;
        // low-resolution pixel (y, x0 + j) of phase (a, b) is output pixel (2 y + a, 2 (x0 + j) + b): stride 2 along the row
        mb[i] = (img * p.Ho + 2 * y + ph_a) * p.Wo + 2 * x0 + ph_b;
        nv[i] = (y < p.H) ? colsv : 0;
    }
    float* epi = reinterpret_cast<float*>(lds) + wave * 32 * (WTN + 4);
    // fused GroupNorm statistics: the 16-bit phase form's slots, [N][tiles][2][4 phases][G][2]
    const int64_t slot = ((int64_t)(img * per_img + trem) * 2 + wm) * 4 + phase;
    float* gn_dst = p.gn_partial ? p.gn_partial + slot * p.gn_entries * 2 : nullptr;
    igemm_epilogue<T, WTN, FM, FN>(p, acc, epi, lane, mb, nv, n0 + wn * WTN, 0, gn_dst, 0, 2, 0);
}

// Block orders: those of igemm_halo_kernel<TAPS = 4> (IgemmGeo.interleave; the chunked per-XCD order is the default)
__global__ __launch_bounds__(256, 2) void mxfp8_conv_up_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    int tile, phase;
    if (g.interleave) {
        if (!phase_block_map((int)blockIdx.x, g.ntm * g.ntn, 0, g.interleave == 2, tile, phase)) return;
    } else {
        tile = xcd_remap((int)blockIdx.x, g.ntm * g.ntn); phase = (int)blockIdx.y;
    }
    mxfp8_conv_up_body(p, g, tile, phase);
}

// Several problems that share the weight, its scales, Cin / Cout and the epilogue options in ONE launch (the tile-shape groups of a tiled-VAE
// layer; timing variant 26): HaloMulti as igemm_halo_multi_kernel<TAPS = 4> reads it - the workgroup looks its problem up in the prefix table
// of 8-aligned block ranges (wave-uniform: blockIdx and kernel arguments only), the filler blocks exit, and the body above runs unchanged.
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
    mxfp8_conv_up_body(m.p[s], m.g[s], tile, phase);
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
    return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad_top == 1 && a.pad_left == 1 && a.upsample == 1 && a.Ho == 2 * a.H && a.Wo == 2 * a.W &&
           (a.Cin % 128) == 0 && a.Cin <= MXU_MAX_CIN && a.K_pad == 9 * a.Cin && (a.in_ld == 0 || a.in_ld == a.Cin) && (a.Cout_pad % BN) == 0 &&
           a.Cout >= 96 && (a.Cout & 7) == 0 && a.act != OMGSR_ACT_GEGLU && a.out_layout == OMGSR_LAYOUT_NHWC && a.batch == 1 && !a.in_split && !a.w_split &&
           a.mx_chunks16 == 0 && a.out_mx == 0 && a.out_lo_off == 0 && !a.gn_scale_shift && !a.residual && a.mxf8 == 0 && compute_dtype() == 0;
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
