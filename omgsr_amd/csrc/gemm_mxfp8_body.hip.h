// Body of mxfp8_gemm_kernel (gemm_mxfp8.hip describes the schedule), shared by its two instantiations: the 16-bit / fp32 output forms
// (gemm_mxfp8.hip) and OUT8, whose epilogue writes the OMGSR_EL_MXFP8 form (gemm_mxfp8_out8.hip: a translation unit of its own, like
// igemm_halo_out6.hip - see igemm_epilogue.hip.h at OUT6 for why an output form is a template flag and not a run-time branch).
// mxfp8_gemm_geglu_kernel (gemm_mxfp8_geglu.hip) instantiates both once more over pack_geglu_weight's interleaved rows, act OMGSR_ACT_GEGLU.
#pragma once
#include "common.hip.h"
#include "../../include/omgsr_hip.h"
#include "timing.hip.h"
#include "igemm_epilogue.hip.h"
#include "igemm_launch.hip.h"
#include "mxfp8.hip.h"
#include <type_traits>

namespace {

constexpr int BM = 256, BN = 256, BK = 128;         // BK in fp8 values = bytes
constexpr int HALF_BYTES = 128 * BK;                // 16 KB
constexpr int BUF_BYTES = 4 * HALF_BYTES;           // A0 A1 B0 B1
constexpr int SC_OFF = 2 * BUF_BYTES;               // per buffer: [A 256 rows x 4 B | B 256 rows x 4 B]
constexpr int SC_BYTES = 2 * 256 * 4;
constexpr int DUMMY_OFF = SC_OFF + 2 * SC_BYTES;
constexpr int LDS_BYTES = DUMMY_OFF + 1024;
constexpr int WTN = 64, FM = 4, FN = 2;

OMGSR_DEVINL void glds16(const unsigned voff, const void* sbase, const unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

OMGSR_DEVINL void glds4(const unsigned voff, const void* sbase, const unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

// `tile`: the workgroup's tile index in the problem's ntm x ntn grid (after xcd_remap), `bz`: its batch index. The single-problem kernels pass
// xcd_remap(blockIdx.x, ...) and blockIdx.z; mxfp8_gemm_multi_kernel (gemm_mxfp8_multi.hip) passes what its lookup found.
template <bool OUT8>
OMGSR_DEVINL void mxfp8_gemm_body(const omgsr_igemm_args& p, const IgemmGeo& g, const int tile, const int bz, const IgemmOut8 o8 = IgemmOut8{nullptr, 0}) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int half = lane >> 5, l31 = lane & 31;

    const int per_group = 8 * g.ntn;
    const int grp = tile / per_group, in_grp = tile - grp * per_group;
    const int first_m = grp * 8;
    const int gsz = (g.ntm - first_m) < 8 ? (g.ntm - first_m) : 8;
    const int tm = first_m + in_grp % gsz, tn = in_grp / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int K = p.Cin;
    const int ksc = K >> 5;                             // scale bytes per row
    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.in) + (int64_t)bz * p.in_bstride;
    const unsigned char* bbase = reinterpret_cast<const unsigned char*>(p.weight) + (int64_t)bz * p.w_bstride;
    const unsigned char* asc = p.in_scale + (int64_t)bz * (p.in_bstride >> 5);
    const unsigned char* bsc = p.w_scale + (int64_t)bz * (p.w_bstride >> 5);
    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;
    const int nkt = K / BK;                             // >= 1

    // ---- prefetch coordinates (igemm_p8_kernel's): piece j of wave w covers rows 16 w + 8 j .. + 7 of a half-tile ----------
    unsigned aoff[2][2], boff[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int rl = 16 * wave + 8 * j + (lane >> 3);
            const int chunk = (lane & 7) ^ ((4 * j + (lane >> 4)) & 7);
            int m = m0 + 128 * h + rl;
            if (m > g.M - 1) m = g.M - 1;
            aoff[h][j] = (unsigned)((int64_t)m * K + chunk * 16);
            boff[h][j] = (unsigned)((int64_t)(n0 + 128 * h + rl) * K + chunk * 16);
        }
    // scale piece: waves 0-3 the operand rows 64 w + lane, waves 4-7 the weight rows 64 (w - 4) + lane (one dword = one K-tile)
    const bool sc_a = wave < 4;
    unsigned scoff;
    {
        int r = 64 * (wave & 3) + lane;
        if (sc_a) {
            r += m0;
            if (r > g.M - 1) r = g.M - 1;
        } else {
            r += n0;
        }
        scoff = (unsigned)((int64_t)r * ksc);
    }
    auto stage = [&](const int buf, const int slot, const int kt) {
        const bool real = kt < nkt;
        const int k = real ? kt : nkt - 1;
        const unsigned char* sb = (slot < 2 ? abase : bbase) + (int64_t)k * BK;
        const unsigned dst = lds_base + buf * BUF_BYTES + slot * HALF_BYTES + (2 * wave) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned vo = slot == 0 ? aoff[0][j] : slot == 1 ? aoff[1][j] : slot == 2 ? boff[0][j] : boff[1][j];
            glds16(vo, sb, __builtin_amdgcn_readfirstlane(real ? dst + j * 1024 : lds_base + DUMMY_OFF));
        }
    };
    auto stage_sc = [&](const int buf, const int kt) {
        const bool real = kt < nkt;
        const int k = real ? kt : nkt - 1;
        const unsigned char* sb = (sc_a ? asc : bsc) + k * 4;
        const unsigned dst = lds_base + SC_OFF + buf * SC_BYTES + wave * 256;
        glds4(scoff, sb, __builtin_amdgcn_readfirstlane(real ? dst : lds_base + DUMMY_OFF));
    };

    // ---- fragment read offsets: k-step s, 16-byte piece e = chunk 4 s + 2 e + h of row l31 (swizzled) ----------------------
    unsigned fa[2][2][2], fb[2][2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const unsigned f = (unsigned)(l31 * 128 + (((4 * s + 2 * e + half) ^ ((l31 >> 1) & 7)) << 4));
                fa[x][s][e] = f + x * BUF_BYTES + wr * HALF_BYTES;
                fb[x][s][e] = f + x * BUF_BYTES + (2 + (wc >> 1)) * HALF_BYTES + (wc & 1) * (64 * 128);
            }
    // scale dwords of the lane's rows: A row wr * 128 + 32 i + l31, B row 64 wc + 32 j + l31
    const unsigned sca = SC_OFF + (wr * 128 + l31) * 4, scb = SC_OFF + 1024 + (64 * wc + l31) * 4;

    f32x16_t acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // ---- prologue: tile 0 (+ its scales) into E, the B half-tiles of tile 1 into O ------------------------------------------
    stage(0, 0, 0); stage(0, 1, 0); stage(0, 2, 0); stage(0, 3, 0); stage_sc(0, 0);
    stage(1, 2, 1); stage(1, 3, 1);
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wr == 1) __builtin_amdgcn_s_barrier();

    i32x8_t a8[2][2], b08[2], b18[2];                   // [ii][s] / [s]
    int sa[2][2], sb0[2], sb1[2];                       // E8M0 operands (byte 0) of the same fragments
    auto ld8 = [&](const unsigned lo, const unsigned hi) {
        return __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(lds + lo), *reinterpret_cast<const i32x4_t*>(lds + hi), 0, 1, 2, 3, 4, 5, 6, 7);
    };
    // the lane's block of k-step s is byte 2 s + h of its row's dword
    auto sbyte = [&](const unsigned w, const int s) { return (int)__builtin_amdgcn_ubfe(w, (unsigned)(16 * s + 8 * half), 8u); };
    auto phase = [&](auto P_c, const int kt, const bool mma) {
        constexpr int P = decltype(P_c)::value, X = P >> 2, q = P & 3;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (q == 0) {
            const unsigned wb = *reinterpret_cast<const unsigned*>(lds + scb + X * SC_BYTES);
            const unsigned w0 = *reinterpret_cast<const unsigned*>(lds + sca + X * SC_BYTES);
            const unsigned w1 = *reinterpret_cast<const unsigned*>(lds + sca + X * SC_BYTES + 32 * 4);
#pragma unroll
            for (int s = 0; s < 2; ++s) b08[s] = ld8(fb[X][s][0], fb[X][s][1]);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int s = 0; s < 2; ++s) a8[ii][s] = ld8(fa[X][s][0] + ii * 4096, fa[X][s][1] + ii * 4096);
#pragma unroll
            for (int s = 0; s < 2; ++s) { sb0[s] = sbyte(wb, s); sa[0][s] = sbyte(w0, s); sa[1][s] = sbyte(w1, s); }
        } else if constexpr (q == 1) {
            const unsigned wb = *reinterpret_cast<const unsigned*>(lds + scb + X * SC_BYTES + 32 * 4);
#pragma unroll
            for (int s = 0; s < 2; ++s) b18[s] = ld8(fb[X][s][0] + 4096, fb[X][s][1] + 4096);
#pragma unroll
            for (int s = 0; s < 2; ++s) sb1[s] = sbyte(wb, s);
        } else if constexpr (q == 2) {
            const unsigned w0 = *reinterpret_cast<const unsigned*>(lds + sca + X * SC_BYTES + 64 * 4);
            const unsigned w1 = *reinterpret_cast<const unsigned*>(lds + sca + X * SC_BYTES + 96 * 4);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int s = 0; s < 2; ++s) a8[ii][s] = ld8(fa[X][s][0] + (2 + ii) * 4096, fa[X][s][1] + (2 + ii) * 4096);
#pragma unroll
            for (int s = 0; s < 2; ++s) { sa[0][s] = sbyte(w0, s); sa[1][s] = sbyte(w1, s); }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (P == 0) stage(1, 0, kt + 1);
        else if constexpr (P == 1) { stage(1, 1, kt + 1); stage_sc(1, kt + 1); }
        else if constexpr (P == 2) stage(0, 2, kt + 2);
        else if constexpr (P == 3) stage(0, 3, kt + 2);
        else if constexpr (P == 4) stage(0, 0, kt + 2);
        else if constexpr (P == 5) { stage(0, 1, kt + 2); stage_sc(0, kt + 2); }
        else if constexpr (P == 6) stage(1, 2, kt + 3);
        else stage(1, 3, kt + 3);
        // 4th / 8th phase: everything but the two youngest half-tiles (4 pieces, issued in the two phases before) has landed - the other
        // buffer, its scale dwords included (staged one phase earlier still), is complete
        if constexpr (q == 3) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (mma) {
            __builtin_amdgcn_s_setprio(1);
            constexpr int i0 = (q >= 2) ? 2 : 0;
            constexpr int j = (q == 1 || q == 2) ? 1 : 0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
                    // inline asm (the builtin lets the allocator move the tied accumulators); s_nop 3: hipcc pads no hazards around inline asm,
                    // and the scale operands are VALU results
                    asm volatile("s_nop 3\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                                 : "+v"(acc[i0 + ii][j]) : "v"(j ? b18[s] : b08[s]), "v"(a8[ii][s]), "v"(j ? sb1[s] : sb0[s]), "v"(sa[ii][s]));   // transposed tile
            __builtin_amdgcn_s_setprio(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    for (int kt = 0; kt < nkt; kt += 2) {
        const bool second = kt + 1 < nkt;               // the O half of this pair holds a real K-tile
        phase(std::integral_constant<int, 0>{}, kt, true);
        phase(std::integral_constant<int, 1>{}, kt, true);
        phase(std::integral_constant<int, 2>{}, kt, true);
        phase(std::integral_constant<int, 3>{}, kt, true);
        phase(std::integral_constant<int, 4>{}, kt, second);
        phase(std::integral_constant<int, 5>{}, kt, second);
        phase(std::integral_constant<int, 6>{}, kt, second);
        phase(std::integral_constant<int, 7>{}, kt, second);
    }
    // the last asm MFMAs (16 passes each) must have written the accumulators before the epilogue's VALU reads them
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    if (wr == 0) __builtin_amdgcn_s_barrier();          // re-align the groups
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    static_assert(8 * 32 * (WTN + 4) * 4 <= LDS_BYTES, "epilogue staging must fit the allocation");
    float* epi = reinterpret_cast<float*>(lds) + wave * 32 * (WTN + 4);
    igemm_epilogue_linear<bf16_t, WTN, FM, FN, OUT8>(p, g.M, acc, epi, lane, m0 + wr * 128, n0 + wc * WTN, bz, 0, o8);
}

}  // namespace
