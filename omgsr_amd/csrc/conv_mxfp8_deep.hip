// Deep-K form of the MXFP8 x MXFP8 3x3 stride-1 pad-1 convolution (OMGSR-S's opt-in UNet resnet convs on the bf16 tier; omgsr_conv_mxfp8_deep,
// timing variant 27, kind 1).
//
// mxfp8_conv_deep_kernel is mxfp8_conv_body (conv_mxfp8.hip: read that file's header for the schedule, the lane map, the operand and weight
// layouts and the weight-scale loads - all unchanged here, the body is a copy) with the operand SCALE plane staged instead of resident, which
// lifts that kernel's two limits:
//  * Cin % 64 == 0 (not % 128): a pixel's Cin / 32 scale bytes are an even count, so a scale row is only 2-byte aligned (10 bytes at Cin = 320).
//    The one access that is aligned and in bounds at every such Cin is ONE CHUNK's byte pair (blocks 2 cc, 2 cc + 1 of one pixel): a 16-bit
//    load at byte offset pixel * Cin / 32 + 2 cc, whose last byte is at most the row's last byte. Nothing wider is ever read, so no load
//    touches a byte past the plane (the guard-band tests poison what lies there);
//  * Cin up to 2048 (not 512): the LDS holds the scale bytes of a WINDOW of MXD_WINDOW_CHUNKS = 1 chunk (2 blocks x 344-byte rows = 688 bytes),
//    double-buffered: 71680 + 2 x 688 = 73056 bytes whatever Cin is (two workgroups per CU). The byte pair above is also the refill's unit, so a
//    wider window would not save a single load - it would only hold bytes longer - hence W = 1: every chunk boundary is a window boundary.
// Refill (window cc + 1 while window cc is consumed; the window's half is the chunk's parity, a compile-time constant of the unrolled chunk
// pair, so a lane's byte of every (tap, fragment) stays "base register + immediate" with NO per-chunk address arithmetic):
//  * thread t owns patch rows t and t + 256 (< 340): two inline-asm global_load_ushort per thread and chunk, issued by every lane of every
//    wave (rows outside the patch or the image read the image's first pixel and are replaced by zero / not written), so that each wave's
//    vmcnt sees the same count;
//  * tap 3 issues them BEHIND that step's weight slice. In flight then: slice 4, slice 5, the pair. The waits of taps 4 and 5 therefore
//    leave 4 instead of 2 operations outstanding when a refill was issued (the slice each of them needs is still the oldest), and tap 6's
//    unchanged vmcnt(2) - which leaves only slice 7 - covers the pair: the refill has the same two-and-a-half K-steps of latency as a
//    weight slice. Every other wait is mxfp8_conv_body's;
//  * tap 6 writes the four bytes into the idle half after its barrier (that half was last read in chunk cc - 1, which every wave has left
//    by then); the lgkmcnt(0) + barrier of tap 7 publish them, two barriers before chunk cc + 1 reads them;
//  * window 0 is written in the prologue with ordinary loads, as mxfp8_conv_body writes its whole plane.
// Pixels outside the image read the zero page (code 0) and a zero scale byte: exact zeros whatever the planes hold beyond the map.
// Served (omgsr_conv_mxfp8_deep_ok): omgsr_conv_mxfp8_ok's rules with Cin % 64 == 0, Cin <= 2048. The epilogue is the shared one.
#include "igemm_halo_body.hip.h"
#include "timing.hip.h"

namespace {

using MG = HaloGeo<9>;
constexpr int MXD_MAX_CIN = 2048;
constexpr int MXD_WINDOW_CHUNKS = 1;                                             // chunks of operand scales per LDS window (see the header)
constexpr int MXD_SA_OFF = MG::LDS_BYTES, MXD_SA_LD = 344;                       // a window: [2 blocks][patch row], rows padded 340 -> 344
constexpr int MXD_WIN_BYTES = MXD_WINDOW_CHUNKS * 2 * MXD_SA_LD;
constexpr int MXD_LDS_BYTES = MXD_SA_OFF + 2 * MXD_WIN_BYTES;                    // double-buffered
static_assert(MXD_WINDOW_CHUNKS == 1, "the window's half is the chunk's parity");
static_assert(MXD_SA_LD >= MG::PROWS && MG::PROWS <= 512, "scale plane pitch; two patch rows per thread");
static_assert(MXD_LDS_BYTES <= 81920, "two workgroups per CU");

OMGSR_DEVINL u32x4_t gload16(const void* src) {
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}
OMGSR_DEVINL unsigned gload2(const void* src) {             // (zero-extended)
    unsigned v;
    asm volatile("global_load_ushort %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}

// The tile body. `tile`: the problem's logical (XCD-remapped) tile index.
OMGSR_DEVINL void mxfp8_conv_deep_body(const omgsr_igemm_args& p, const IgemmGeo& g, const int tile) {
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

    // operand scales: thread t owns patch rows t and t + 256; s_ptr[e] points at the row's byte pair of the NEXT window (it advances 2 bytes
    // per chunk where the row lies in the image; every other row reads the image's first pixel and counts as zero)
    const unsigned char* s_ptr[2];
    unsigned s_ok = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int pr = t + 256 * e;
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + py, vx = x0 - 1 + px;
        const bool ok = pr < PROWS && (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = (int64_t)img * p.H * p.W + (ok ? vy * p.W + vx : 0);
        s_ptr[e] = p.in_scale + pix * nb;
        s_ok |= (ok ? 1u : 0u) << e;
    }
    unsigned sc[2];
    auto issue_sc = [&]() {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            sc[e] = gload2(s_ptr[e]);
            s_ptr[e] += ((s_ok >> e) & 1u) << 1;
        }
    };
    auto store_sc = [&](const int win) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int pr = t + 256 * e;
            if (pr < PROWS) {
                const unsigned v = ((s_ok >> e) & 1u) ? sc[e] : 0u;
                unsigned char* dst = lds + MXD_SA_OFF + win * MXD_WIN_BYTES + pr;
                dst[0] = (unsigned char)v;
                dst[MXD_SA_LD] = (unsigned char)(v >> 8);
            }
        }
    };
    // window 0 (ordinary loads and ds_writes: the compiler waits for them; the first K-step's barrier publishes them)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        sc[e] = *reinterpret_cast<const unsigned short*>(s_ptr[e]);
        s_ptr[e] += ((s_ok >> e) & 1u) << 1;
    }
    store_sc(0);
    // a lane's scale byte of fragment i, tap (ky, kx), chunk cc: window half cc & 1, block `half` of patch row (4 wm + i + ky) PW + frow + kx
    const int sa_base = MXD_SA_OFF + half * MXD_SA_LD + FM * wm * PW + frow;

    // one K-step with compile-time tap and patch parity (see halo_body for the wait / barrier / late-issue reasoning, unchanged here)
    auto step = [&](auto tap_c, auto par_c, const int cc, const int s) {
        constexpr int tap = decltype(tap_c)::value, par = decltype(par_c)::value;
        if constexpr (tap == 1) {
            if (cc + 1 < ncc) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        } else if constexpr (tap == 4 || tap == 5) {
            // tap 3 issued the next window's scale pair (2) behind its weight slice: it is still in flight next to the younger slice
            if (cc + 1 < ncc) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
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
        if constexpr (tap == 6) {
            // the wait above left only tap 7's slice in flight: the scale pair issued at tap 3 has landed; the idle half was last read in
            // chunk cc - 1
            if (cc + 1 < ncc) {
                asm volatile("" : "+v"(sc[0]), "+v"(sc[1]));
                store_sc(par ^ 1);
            }
        }
        auto issue_dma = [&]() {
            if constexpr (tap == 0) { if (cc + 1 < ncc) issue_a(par ^ 1); }
            if constexpr (tap == TAPS - 1) { if (cc + 1 < ncc) issue_ws(); }        // (this step's own bytes were extracted above)
            if (s + 2 < nsteps) issue_b((tap + 2) % NB);
            if constexpr (tap == 3) { if (cc + 1 < ncc) issue_sc(); }
        };

        const unsigned char* As = lds + par * A_BYTES;
        const unsigned char* Bs = lds + B_OFF + (tap % NB) * B_BYTES;
        const unsigned char* Ss = lds + sa_base + par * MXD_WIN_BYTES;
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

__global__ __launch_bounds__(256, 2) void mxfp8_conv_deep_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    mxfp8_conv_deep_body(p, g, xcd_remap((int)blockIdx.x, g.ntm * g.ntn));
}

}  // namespace

namespace omgsr {
// What mxfp8_conv_deep_kernel itself needs (the dispatcher-side half of omgsr_conv_mxfp8_deep_ok - "the bf16 path would take the spatial
// nine-tap form" - lives next to that dispatcher in igemm.hip): mxfp8_conv_shape_ok's rules with the two Cin limits replaced
bool mxfp8_conv_deep_shape_ok(const omgsr_igemm_args& a) {
    return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad_top == 1 && a.pad_left == 1 && a.upsample == 0 && a.Ho == a.H && a.Wo == a.W &&
           (a.Cin % 64) == 0 && a.Cin > 0 && a.Cin <= MXD_MAX_CIN && a.K_pad == 9 * a.Cin && (a.in_ld == 0 || a.in_ld == a.Cin) && (a.Cout_pad % BN) == 0 &&
           a.Cout >= 96 && a.act != OMGSR_ACT_GEGLU && a.out_layout == OMGSR_LAYOUT_NHWC && a.batch == 1 && !a.in_split && !a.w_split &&
           a.mx_chunks16 == 0 && a.out_mx == 0 && a.out_lo_off == 0 && !a.gn_scale_shift && !a.weight_ph && a.mxf8 == 0 && compute_dtype() == 0;
}

int mxfp8_conv_deep_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st, const double flops) {
    const bool narrow = halo_geo(a, g, false);
    if (narrow || g.flat) return OMGSR_E_SHAPE;               // (omgsr_conv_mxfp8_deep_ok refused both: never reached)
    const double M = (double)a.N * a.Ho * a.Wo;
    const double bytes = (1.0 + 1.0 / 32.0) * ((double)a.N * a.H * a.W * a.Cin + (double)a.Cout_pad * a.K_pad) +
                         M * a.Cout * ((a.out_dtype == OMGSR_OUT_F32 ? 4.0 : 2.0) + (a.residual ? (a.res_el == OMGSR_EL_F32 ? 4.0 : 2.0) : 0.0));
    TimingScope ts(OMGSR_TK_IGEMM, flops, bytes, st, (long long)M, a.Cout, 9ll * a.Cin);
    if (ts.active) ts.rec.variant = 27;
    return launch_lds<mxfp8_conv_deep_kernel>(dim3(g.ntm * g.ntn), dim3(256), MXD_LDS_BYTES, st, a, g);
}
}  // namespace omgsr
