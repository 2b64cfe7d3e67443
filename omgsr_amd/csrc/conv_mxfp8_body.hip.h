// The one tile body of the MXFP8 x MXFP8 halo convolutions: conv_mxfp8.hip (<9, false>: nine taps, resident operand scales), conv_mxfp8_deep.hip
// (<9, true>: nine taps, windowed operand scales) and conv_mxfp8_up.hip (<4, false>: the four-tap phase form of nearest-2x up-sampling + conv).
//
// The body runs the halo-tile schedule of igemm_halo_body.hip.h (8 x 32-pixel x 128-cout tile, patch LDS-DMA'd once per chunk and read by
// every tap at shifted rows, weight ring, one raw barrier and one counted vmcnt wait per K-step) on fp8 codes:
//  * a chunk is 64 e4m3 channels = the same 64-byte patch rows and 8 KB weight slices as a 32-channel bf16 chunk, so patch geometry, DMA pieces
//    and the vmcnt arithmetic are the bf16 kernel's, while a K-step is one v_mfma_scale_f32_32x32x64_f8f6f4 per fragment pair (16 passes)
//    where bf16 issues two 32x32x16 of 8: the same matrix-pipe time for twice the contraction;
//  * operand: OMGSR_EL_MXFP8 as omgsr_quantize_mxfp8 / omgsr_groupnorm_apply_mxfp8 write it, rows = pixels: codes [N][H][W][Cin], scales
//    [N][H][W][Cin / 32]. Pixels outside the map read the zero page (code 0) and a zero scale byte: exact zeros whatever the planes hold
//    beyond the map;
//  * lane map (measured): lane l = (row l & 31, half h = l >> 5) holds K 16 h .. + 15 (registers 0-3) and 32 + 16 h .. + 15
//    (registers 4-7) of the 64, and the scale of hardware block b (K 32 b .. + 31 = the format's block 2 cc + b of chunk cc) is taken from lane
//    half b: a lane's two 16-byte reads are the row's 16-byte pieces h and 2 + h (as in the bf16 kernel), and it supplies the E8M0 byte of
//    block 2 cc + h of ITS row on both sides;
//  * column swizzle: patch rows are swizzled by their patch COLUMN ((px >> 2) & 3) where halo_body swizzles by the patch row index. 16
//    consecutive pixels of a tile row still hit 16 distinct 16-byte slots, and a fragment's address becomes (tile row) x pitch + f(column)
//    with the tile-row term an immediate of the ds_read: KW address registers (one per tap column) serve all (tap, fragment) pairs - 3 instead
//    of 18 in the nine-tap form, which is what fits the scale registers into 256 VGPRs without spilling;
//  * weight scales: a lane fetches the scale bytes of its two weight rows for a WHOLE chunk (one group of WS_GROUP bytes per row, byte t =
//    tap t) with plain global loads into single-buffered registers (a double buffer spills), issued in the last K-step of the previous chunk
//    behind that step's MFMAs and IN FRONT of its weight slice; the tap's byte is shifted down with v_bfe;
//  * inline-asm loads: everything the K loop fetches (LDS-DMA pieces, weight scales, the windowed operand scales) is inline asm. A
//    compiler-tracked load would make hipcc insert vmcnt(0) at its first use and drain the prefetched patch. The loaded registers pass
//    through an empty asm after the wait that covers them, so that no use can be scheduled in front of it;
//  * counted waits (every wave issues the same operations, dummy pieces included, so the counts are uniform): a step waits until only what
//    the PREVIOUS step issued may be in flight - its weight slice, 2 pieces per wave: vmcnt(2). Tap 0 also issued the next chunk's patch
//    (APW pieces), so tap 1 leaves APW + 2; the weight scales sit in front of the last tap's slice, so tap 0's vmcnt(2) covers them; the
//    last step of the tile drains with vmcnt(0). lgkmcnt(0) rides every wait: the previous step's fragment reads have returned before the
//    barrier lets another wave's DMA overwrite that stage (igemm_halo_body.hip.h has the history);
//  * late issue: a step's DMA is issued between the two halves of its MFMAs, so its issue slots overlap matrix-pipe time. The stage it fills
//    was last read in the previous step, which every wave left at this step's barrier;
//  * the asm MFMAs are invisible to the compiler's hazard padding: s_nop 3 in front of each (its scale operands are VALU / LDS results),
//    two s_nop 7 in front of the loop, six s_nop 15 between the last MFMA (16 passes) and the epilogue's reads of the accumulators.
//
// Axis 1, TAPS. 9 (HaloGeo<9>): 3 x 3 taps of a 10 x 34 = 340-row patch in 22 pieces, 6 per wave (tap 1 waits vmcnt(8)), 3-deep weight ring,
// `weight_cm` uint8 [Cin / 64][9][Cout_pad][64], `w_scale` uint8 [Cin / 64][Cout_pad][2 blocks][16] (bytes 9-15 zero): a dwordx4 per row.
// 4 (HaloGeo<4>): phase 2 a + b of the up-sampled output is a 2 x 2 convolution of the LOW-resolution map (rows y - 1 + a, y + a; columns
// likewise) with phase-summed weights: 9 x 33 = 297-row patch in 19 pieces, 5 per wave (tap 1 waits vmcnt(7)), 4-deep ring (stage = tap),
// `weight_ph` uint8 [4 phases][Cin / 64][4][Cout_pad][64], `w_scale` uint8 [4 phases][Cin / 64][Cout_pad][2 blocks][4]: a dword per row; the
// tile's outputs land at stride 2 in the high-resolution map and the GroupNorm partials take the phase form's slots.
//
// Axis 2, WINDOWED. false (resident): the whole patch's scale bytes ([Cin / 32 blocks][SA_LD], block-major so that a lane's byte of every
// (tap, fragment) is one per-chunk base register plus an immediate) are copied into LDS once per tile behind the weight ring, with whole-dword
// loads: Cin % 128 == 0, and Cin bounded by the LDS the plane takes. true: the LDS holds a WINDOW of one chunk (2 blocks x SA_LD bytes),
// double-buffered, whatever Cin is, and Cin % 64 == 0 suffices: a pixel's Cin / 32 scale bytes are then an even count, so a scale row is only
// 2-byte aligned (10 bytes at Cin = 320), and the one access that is aligned and in bounds at every such Cin is ONE CHUNK's byte pair (blocks
// 2 cc, 2 cc + 1 of one pixel): a 16-bit load at byte offset pixel * Cin / 32 + 2 cc, whose last byte is at most the row's last byte. Nothing
// wider is ever read, so no load touches a byte past the plane (the guard-band tests poison what lies there). The byte pair is also the
// refill's unit, so a wider window would not save a single load - it would only hold bytes longer - hence 1 chunk: every chunk boundary is
// a window boundary.
// Refill (window cc + 1 while window cc is consumed; the window's half is the chunk's parity, a compile-time constant of the unrolled chunk
// pair, so a lane's byte of every (tap, fragment) stays "base register + immediate" with NO per-chunk address arithmetic):
//  * thread t owns patch rows t and t + 256 (< 340): two inline-asm global_load_ushort per thread and chunk, issued by every lane of every
//    wave (rows outside the patch or the image read the image's first pixel and are replaced by zero / not written), so that each wave's
//    vmcnt sees the same count;
//  * tap 3 issues them BEHIND that step's weight slice. In flight then: slice 4, slice 5, the pair. The waits of taps 4 and 5 therefore
//    leave 4 instead of 2 operations outstanding when a refill was issued (the slice each of them needs is still the oldest), and tap 6's
//    unchanged vmcnt(2) - which leaves only slice 7 - covers the pair: the refill has the same two-and-a-half K-steps of latency as a
//    weight slice. Every other wait is the resident form's;
//  * tap 6 writes the four bytes into the idle half after its barrier (that half was last read in chunk cc - 1, which every wave has left
//    by then); the lgkmcnt(0) + barrier of tap 7 publish them, two barriers before chunk cc + 1 reads them;
//  * window 0 is written in the prologue with ordinary loads, as the resident form writes its whole plane.
#pragma once
#include "igemm_halo_body.hip.h"

namespace {

OMGSR_DEVINL u32x4_t gload16(const void* src) {
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}
OMGSR_DEVINL unsigned gload4(const void* src) {
    unsigned v;
    asm volatile("global_load_dword %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}
OMGSR_DEVINL unsigned gload2(const void* src) {             // (zero-extended)
    unsigned v;
    asm volatile("global_load_ushort %0, %1, off" : "=&v"(v) : "v"(src) : "memory");
    return v;
}
template <int N> OMGSR_DEVINL void wait_vm() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(N) : "memory"); }

// What follows from the two axes
template <int TAPS, bool WINDOWED> struct Mxfp8ConvTraits {
    static_assert(TAPS == 9 || TAPS == 4, "nine taps or the four-tap phase form");
    static_assert(!(WINDOWED && TAPS == 4), "the windowed phase form is not built: the refill timeline is written for nine taps");
    using Geo = HaloGeo<TAPS>;
    static constexpr bool PHASED = TAPS == 4;
    static constexpr int KW = Geo::KS;                                           // taps per patch row: tap = KW * (row) + (column)
    static constexpr int SA_OFF = Geo::LDS_BYTES, SA_LD = (Geo::PROWS + 7) & ~7;  // operand scale bytes: [block][patch row], rows padded 340 -> 344, 297 -> 304
    static constexpr int WINDOW_CHUNKS = 1, WIN_BYTES = WINDOW_CHUNKS * 2 * SA_LD;
    static constexpr int WS_GROUP = PHASED ? 4 : 16;                             // weight-scale bytes per (chunk, cout, block)
    using ws_t = std::conditional_t<PHASED, unsigned, u32x4_t>;
    // the type of a local that only the windowed form has (empty in the resident form). Plain locals, not one struct: hipcc numbers the deep
    // kernel's prologue registers differently for a struct, and the three units are held to the assembly of the copies they replaced
    struct Absent {};
    template <typename A> using windowed_t = std::conditional_t<WINDOWED, A, Absent>;
    static constexpr int lds_bytes(const int max_cin) { return SA_OFF + (WINDOWED ? 2 * WIN_BYTES : SA_LD * (max_cin / 32)); }
    static_assert(SA_LD >= Geo::PROWS && (!WINDOWED || Geo::PROWS <= 512), "scale plane pitch; windowed: two patch rows per thread");
};

// The tile body. `tile`: the problem's logical tile index (on the LOW-resolution grid in the phase form), `phase` = 2 a + b (nine taps: 0).
template <int TAPS, bool WINDOWED>
OMGSR_DEVINL void mxfp8_conv_tile(const omgsr_igemm_args& p, const IgemmGeo& g, const int tile, const int phase) {
    using T = bf16_t;
    using X = Mxfp8ConvTraits<TAPS, WINDOWED>;
    using HG = typename X::Geo;
    constexpr bool PHASED = X::PHASED;
    constexpr int WTN = 64, FM = 4, FN = 2, BNK = 128, KW = X::KW, SA_OFF = X::SA_OFF, SA_LD = X::SA_LD, WIN_BYTES = X::WIN_BYTES, WSG = X::WS_GROUP;
    constexpr int PW = HG::PW, PROWS = HG::PROWS, APIECES = HG::APIECES, APW = HG::APW, A_BYTES = HG::A_BYTES;
    constexpr int NB = HG::NB, DUMMY_OFF = HG::DUMMY_OFF, B_OFF = HG::B_OFF;
    static_assert(TAPS % NB == 0 && NB >= 3, "ring stage = tap % NB; a slice is issued two steps ahead");
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int ph_a = PHASED ? phase >> 1 : 0, ph_b = PHASED ? phase & 1 : 0;

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
    const unsigned char* __restrict__ wt = PHASED ? reinterpret_cast<const unsigned char*>(p.weight_ph) + (int64_t)phase * ncc * TAPS * p.Cout_pad * 64
                                                  : reinterpret_cast<const unsigned char*>(p.weight_cm);
    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;

    const int lrow = lane >> 2;
    const int kc = (lane & 3) ^ ((lane >> 4) & 3);           // weight slices: source piece for LDS position (lane & 3), swizzled by the row as in halo_body

    // patch pieces: piece j = wave * APW + i covers patch rows [16 j, 16 j + 16); patch row -> (py, px)
    const unsigned char* a_ptr[APW];
    unsigned a_ok = 0;                                       // bit i: piece i of this lane lies in the map (its pointer advances 64 bytes per chunk)
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int pr = 16 * (wave * APW + i) + lrow;
        const int py = pr / PW, px = pr - py * PW;
        const int vy = y0 - 1 + ph_a + py, vx = x0 - 1 + ph_b + px;
        const bool ok = (wave * APW + i) < APIECES && pr < PROWS && (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
        const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
        const int kca = (lane & 3) ^ ((px >> 2) & 3);          // the column swizzle
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
    // weight scales of the lane's two rows (cout n0 + 64 wn + 32 j + frow, block `half`), one WSG-byte group per chunk
    const unsigned char* ws_ptr = (PHASED ? p.w_scale + (int64_t)phase * ncc * p.Cout_pad * (2 * WSG) : p.w_scale) + ((int64_t)(n0 + wn * WTN + frow) * 2 + half) * WSG;
    const int64_t ws_step = (int64_t)p.Cout_pad * (2 * WSG);
    typename X::ws_t ws[FN];
    auto issue_ws = [&]() {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            if constexpr (PHASED) ws[j] = gload4(ws_ptr + j * (32 * 2 * WSG));
            else ws[j] = gload16(ws_ptr + j * (32 * 2 * WSG));
        }
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
    // fragment i of tap (ky, kx): patch row (4 wm + i + ky) PW + frow + kx = aoff[kx] + (i + ky) PW 64 (an immediate; a multiple of 64, so it
    // leaves the 16-byte slot bits - the swizzle and the ^ 32 that selects the lane's second piece - alone)
    int aoff[KW];
#pragma unroll
    for (int kx = 0; kx < KW; ++kx) aoff[kx] = (FM * wm * PW + frow + kx) * 64 + ((half ^ (((frow + kx) >> 2) & 3)) << 4);

    issue_ws();
    issue_a(0);
    issue_b(0);
    issue_b(1);

    // the operand scales of the first chunk (windowed) or of all chunks (resident) -> LDS (ordinary loads and ds_writes: the compiler waits for
    // them; the first K-step's barrier publishes them)
    // windowed: thread t owns patch rows t and t + 256; s_ptr[e] points at the row's byte pair of the NEXT window (it advances 2 bytes per chunk
    // where the row lies in the image - bit e of s_ok; every other row reads the image's first pixel and counts as zero); sc: the pair in flight.
    // The two lambdas take them as arguments so that the resident form, which has none of the three, never instantiates them
    typename X::template windowed_t<const unsigned char* [2]> s_ptr;
    typename X::template windowed_t<unsigned> s_ok{};
    typename X::template windowed_t<unsigned[2]> sc;
    auto issue_sc = [&](auto& ptr, auto& ok, auto& pair) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            pair[e] = gload2(ptr[e]);
            ptr[e] += ((ok >> e) & 1u) << 1;
        }
    };
    auto store_sc = [&](auto& ok, auto& pair, const int win) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int pr = t + 256 * e;
            if (pr < PROWS) {
                const unsigned v = ((ok >> e) & 1u) ? pair[e] : 0u;
                unsigned char* dst = lds + SA_OFF + win * WIN_BYTES + pr;
                dst[0] = (unsigned char)v;
                dst[SA_LD] = (unsigned char)(v >> 8);
            }
        }
    };
    if constexpr (WINDOWED) {
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
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            sc[e] = *reinterpret_cast<const unsigned short*>(s_ptr[e]);
            s_ptr[e] += ((s_ok >> e) & 1u) << 1;
        }
        store_sc(s_ok, sc, 0);
    } else {
        for (int pr = t; pr < PROWS; pr += 256) {
            const int py = pr / PW, px = pr - py * PW;
            const int vy = y0 - 1 + ph_a + py, vx = x0 - 1 + ph_b + px;
            const bool ok = (unsigned)vy < (unsigned)p.H && (unsigned)vx < (unsigned)p.W;
            const int64_t pix = ((int64_t)img * p.H + vy) * p.W + vx;
            const unsigned* src = reinterpret_cast<const unsigned*>(p.in_scale + pix * nb);
            unsigned char* dst = lds + SA_OFF + pr;
            for (int q = 0; q < (nb >> 2); ++q) {
                const unsigned w = ok ? src[q] : 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(4 * q + e) * SA_LD] = (unsigned char)(w >> (8 * e));
            }
        }
    }
    // a lane's scale byte of fragment i, tap (ky, kx), chunk cc: block 2 cc + half (windowed: window half cc & 1, block `half`) of patch row
    // (4 wm + i + ky) PW + frow + kx
    const int sa_base = SA_OFF + half * SA_LD + FM * wm * PW + frow;

    // one K-step with compile-time tap and patch parity
    auto step = [&](auto tap_c, auto par_c, const int cc, const int s) {
        constexpr int tap = decltype(tap_c)::value, par = decltype(par_c)::value;
        if constexpr (tap == 1) {
            // the previous step (tap 0) issued the next chunk's patch (APW pieces) and one weight slice (2)
            if (cc + 1 < ncc) wait_vm<APW + 2>();
            else wait_vm<2>();
        } else if constexpr (WINDOWED && (tap == 4 || tap == 5)) {
            // tap 3 issued the next window's scale pair (2) behind its weight slice: it is still in flight next to the younger slice
            if (cc + 1 < ncc) wait_vm<4>();
            else wait_vm<2>();
        } else if constexpr (tap == TAPS - 1) {
            if (s + 1 < nsteps) wait_vm<2>();
            else wait_vm<0>();
        } else {
            wait_vm<2>();
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (tap == 0) {
            // this chunk's weight scales were issued in the previous step (or the prologue) in front of its weight slice: the wait above,
            // which leaves only that slice in flight, covers them
#pragma unroll
            for (int j = 0; j < FN; ++j) asm volatile("" : "+v"(ws[j]));
        }
        if constexpr (WINDOWED) {
            // tap 6: the wait above left only tap 7's slice in flight: the scale pair issued at tap 3 has landed; the idle half was last read in
            // chunk cc - 1
            if constexpr (tap == 6) {
                if (cc + 1 < ncc) {
                    asm volatile("" : "+v"(sc[0]), "+v"(sc[1]));
                    store_sc(s_ok, sc, par ^ 1);
                }
            }
        }
        auto issue_dma = [&]() {
            if constexpr (tap == 0) { if (cc + 1 < ncc) issue_a(par ^ 1); }
            if constexpr (tap == TAPS - 1) { if (cc + 1 < ncc) issue_ws(); }        // (this step's own bytes were extracted above)
            if (s + 2 < nsteps) issue_b((tap + 2) % NB);
            if constexpr (WINDOWED) { if constexpr (tap == 3) { if (cc + 1 < ncc) issue_sc(s_ptr, s_ok, sc); } }
        };

        constexpr int ky = tap / KW, kx = tap % KW;
        const unsigned char* As = lds + par * A_BYTES;
        const unsigned char* Bs = lds + B_OFF + (tap % NB) * B_BYTES;
        const unsigned char* Ss = lds + sa_base + (WINDOWED ? par * WIN_BYTES : (2 * cc) * SA_LD);
        i32x8_t a8[FM], b8[FN];
        int sa[FM], sb[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            a8[i] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(As + (i + ky) * PW * 64 + aoff[kx]),
                                            *reinterpret_cast<const i32x4_t*>(As + (i + ky) * PW * 64 + (aoff[kx] ^ 32)), 0, 1, 2, 3, 4, 5, 6, 7);
            sa[i] = Ss[(i + ky) * PW + kx];                     // (an immediate offset of the ds_read: no address arithmetic in the loop)
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            b8[j] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff0), *reinterpret_cast<const i32x4_t*>(Bs + j * 32 * 64 + boff1),
                                            0, 1, 2, 3, 4, 5, 6, 7);
            if constexpr (PHASED) sb[j] = (int)__builtin_amdgcn_ubfe(ws[j], (unsigned)(8 * tap), 8u);
            else sb[j] = (int)__builtin_amdgcn_ubfe(ws[j][tap >> 2], (unsigned)(8 * (tap & 3)), 8u);
        }
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
            for (int j = 0; j < FN; ++j)
                // inline asm keeps the tied accumulators in place
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
        if constexpr (TAPS == 9) {
            step(std::integral_constant<int, 4>{}, par_c, cc, s0 + 4);
            step(std::integral_constant<int, 5>{}, par_c, cc, s0 + 5);
            step(std::integral_constant<int, 6>{}, par_c, cc, s0 + 6);
            step(std::integral_constant<int, 7>{}, par_c, cc, s0 + 7);
            step(std::integral_constant<int, 8>{}, par_c, cc, s0 + 8);
        }
    };
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    for (int cc = 0; cc < ncc; cc += 2) {
        chunk(std::integral_constant<int, 0>{}, cc);
        if (cc + 1 < ncc) chunk(std::integral_constant<int, 1>{}, cc + 1);
    }
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");

    // the tile's rows in the output map (the phase form's tile is in low-resolution coordinates: its pixel (y, x0 + j) of phase (a, b) is output
    // pixel (2 y + a, 2 (x0 + j) + b), stride 2 along the row) and its GroupNorm statistic slot: (spatial tile, upper / lower 4 tile rows),
    // [N][2 * tiles][G][2] - the bf16 halo kernel's layout - or the 16-bit phase form's [N][tiles][2][4 phases][G][2]
    int mb[FM], nv[FM];
    int colsv = (PHASED ? p.W : p.Wo) - x0; colsv = colsv > TW ? TW : colsv;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int y = y0 + FM * wm + i;
        mb[i] = PHASED ? (img * p.Ho + 2 * y + ph_a) * p.Wo + 2 * x0 + ph_b : (img * p.Ho + y) * p.Wo + x0;
        nv[i] = (y < (PHASED ? p.H : p.Ho)) ? colsv : 0;
    }
    float* epi = reinterpret_cast<float*>(lds) + wave * 32 * (WTN + 4);
    const int64_t slot = PHASED ? ((int64_t)(img * per_img + trem) * 2 + wm) * 4 + phase : (int64_t)(img * per_img + trem) * 2 + wm;
    float* gn_dst = p.gn_partial ? p.gn_partial + slot * p.gn_entries * 2 : nullptr;
    igemm_epilogue<T, WTN, FM, FN>(p, acc, epi, lane, mb, nv, n0 + wn * WTN, 0, gn_dst, 0, PHASED ? 2 : 1, 0);
}

// The shape clauses every form shares (each form's own: its Cin modulus and limit, `upsample` and the Ho / Wo relation, and what its file adds)
inline bool mxfp8_conv_common_shape_ok(const omgsr_igemm_args& a) {
    return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad_top == 1 && a.pad_left == 1 && a.K_pad == 9 * a.Cin && (a.in_ld == 0 || a.in_ld == a.Cin) &&
           (a.Cout_pad % BN) == 0 && a.Cout >= 96 && a.act != OMGSR_ACT_GEGLU && a.out_layout == OMGSR_LAYOUT_NHWC && a.batch == 1 && !a.in_split &&
           !a.w_split && a.mx_chunks16 == 0 && a.out_mx == 0 && a.out_lo_off == 0 && !a.gn_scale_shift && a.mxf8 == 0 && omgsr::compute_dtype() == 0;
}

// Bytes moved, for the timing scope, of the nine-tap forms: one problem's operand + output (+ residual), and the weight with its scales
// (every term is a whole number of 32nds, exact in a double: the sums do not depend on their order)
inline double conv9_bytes(const omgsr_igemm_args& a) {
    const double M = (double)a.N * a.Ho * a.Wo;
    return (1.0 + 1.0 / 32.0) * (double)a.N * a.H * a.W * a.Cin +
           M * a.Cout * ((a.out_dtype == OMGSR_OUT_F32 ? 4.0 : 2.0) + (a.residual ? (a.res_el == OMGSR_EL_F32 ? 4.0 : 2.0) : 0.0));
}
inline double conv9_weight_bytes(const omgsr_igemm_args& a) { return (1.0 + 1.0 / 32.0) * (double)a.Cout_pad * a.K_pad; }

}  // namespace
