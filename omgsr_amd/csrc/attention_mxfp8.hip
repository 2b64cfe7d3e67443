// MXFP8 joint attention (ABI v19, omgsr_attn_args.qkv_el = OMGSR_EL_MXFP8): softmax(Q K^T * scale) V for head_dim 128 with q, k and V^T in
// the OMGSR_EL_MXFP8 form and both products on v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, fp32 accumulate) - the fp8 tier's opt-in
// `fp8_attention`. attn_kernel's schedule (attention.hip) on fp8 codes:
//  * one workgroup = 4 waves = 128 queries, a wave owns 32 queries for the whole key sweep; 64-key K / V^T tiles double-buffered in LDS by
//    LDS-DMA (global_load_lds_dwordx4, one barrier per tile); 1-D grid in XCD order; Q fragments and their scales in registers.
//  * S^T = K Q^T: two instructions (head-dim halves) per 32-key score block. Operand map of the instruction (e4m3): lane half
//    h holds K slots 16h .. 16h + 15 in registers 0-3 and 32 + 16h .. in registers 4-7, and the scale of K block b comes from lane half b.
//    K rows are read through the permutation pi (key bits [b0 b1 b3 b4 b2] of row i), so C register r of lane half h holds key 16h + r of the
//    score block: a lane's 16 scores of a block are 16 CONSECUTIVE keys.
//  * O^T = V^T P^T: one instruction per 32 channels and 64-key tile. The P^T operand is the score registers converted in place: registers
//    0-3 of both lane halves hold score block 0 (keys 0 .. 31), registers 4-7 block 1, so each MX block of the product is 32 consecutive keys -
//    the block the quantiser writes for V^T - and a lane's V^T fragment is two 16-byte LDS reads.
//  * P rule (fixed; omgsr_amd.testing.mxfp8_attention_ref restates it): exact running maximum, codes = e4m3(P 2^8) (round to nearest even,
//    P 2^8 in [0, 256]), scale byte 119 = 2^-8; probabilities down to ~2^-17 of the row maximum survive. The row sum l adds the DEQUANTISED
//    P that enters the PV product - as a fifth scaled MFMA per tile (all-ones A operand), not on the VALU, which limits the kernel - so O is
//    an exact weighted mean of V's rows in the kernel's arithmetic (a constant V comes out unchanged).
//  * keys >= Lk: k rows are clamped to Lk - 1 (never read past the operand), their scores are -inf, the V^T codes there are zeroed and a V^T
//    block wholly past Lk gets scale 2^0: padding of any content cannot reach the result. Only a partial last tile pays for that: it runs the
//    masked instantiation of the tile body once after the loop over whole tiles, which carries no mask and no per-lane address arithmetic.
// Every reduction is lane-local in a fixed order plus one exchange with lane ^ 32: the same launch gives the same bits, and a row's result
// does not depend on the batch.
#include "common.hip.h"
#include "../../include/omgsr_hip.h"
#include "timing.hip.h"
#include <type_traits>

namespace {

constexpr int D = 128, KT = 64;                     // head dim, keys per tile
constexpr int K_BYTES = KT * D;                     // 64 key rows x 128 codes (128-byte rows)
constexpr int V_BYTES = D * KT;                     // 128 channel rows x 64 key codes (64-byte rows)
constexpr int STAGE = K_BYTES + V_BYTES;
constexpr int LDS_BYTES = 2 * STAGE;                // 32 KB: two workgroups per CU
constexpr int P_SCALE = 119;                        // E8M0 of 2^-8
// A/B builds only (OMGSR_EXTRA_DEFS=-DOMGSR_ATTN_FP8_DEFER=t, 1 <= t <= 8; not shipped, not restated by the emulator): the fast tiers' deferred
// maximum - the running maximum moves only when a row's grows by more than 2^t, codes e4m3(P 2^(8 - t)), scale 2^(t - 8)
#ifndef OMGSR_ATTN_FP8_DEFER
#define OMGSR_ATTN_FP8_DEFER 0
#endif
constexpr int DEFER = OMGSR_ATTN_FP8_DEFER;
static_assert(DEFER >= 0 && DEFER <= 8, "OMGSR_ATTN_FP8_DEFER: 0 .. 8");

OMGSR_DEVINL void glds16_fa(const unsigned voff, const void* sbase, const unsigned lds_dst) {
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

OMGSR_DEVINL f32x16_t mfma_mx8(const i32x8_t a, const i32x8_t b, const f32x16_t c, const int sa, const int sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, sa, 0, sb);     // e4m3 x e4m3, scale byte 0 of each operand
}

// XOR swizzle of the 16-byte slot of a K row (128 B: 8 slots): bits 1, 2, 4 of the row, so the 16 rows pi(0 .. 15) that a quarter-wave reads
// fill the 16 slots of a 256-byte bank row once. V^T rows (64 B: 4 slots): bits 2, 3.
OMGSR_DEVINL int kswz(const int r) { return ((r >> 1) & 3) | ((r >> 2) & 4); }
OMGSR_DEVINL int vswz(const int r) { return (r >> 2) & 3; }

__global__ __launch_bounds__(256, 2) void mxfp8_attn_kernel(const omgsr_attn_args p, const int ntiles, const int qtiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int qt = tile % qtiles, bh = tile / qtiles;
    const int h = bh % p.H, b = bh / p.H;
    const int q0 = qt * 128 + wave * 32;
    const int Lk = p.Lk;

    const unsigned char* __restrict__ qp = (const unsigned char*)p.q + (int64_t)b * p.q_bstride + h * D;
    const unsigned char* __restrict__ kp = (const unsigned char*)p.k + (int64_t)b * p.k_bstride + h * D;
    const unsigned char* __restrict__ vp = (const unsigned char*)p.vt + (int64_t)b * p.vt_bstride + (int64_t)h * D * p.vt_ld;
    const unsigned char* __restrict__ qs = p.q_scale + (int64_t)b * p.q_sbstride + h * (D / 32);
    const unsigned char* __restrict__ ks = p.k_scale + (int64_t)b * p.k_sbstride + h * (D / 32);
    const unsigned char* __restrict__ vs = p.vt_scale + (int64_t)b * p.vt_sbstride + (int64_t)h * D * p.vt_sld;

    // Q^T operand (query q0 + l31, k-step s = head-dim half) and the lane's scale byte of block 2s + half
    i32x8_t qf[2];
    int qsc[2];
    {
        int qrow = q0 + l31;
        if (qrow > p.Lq - 1) qrow = p.Lq - 1;
        const unsigned char* qr = qp + (int64_t)qrow * p.q_ld;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            qf[s] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(qr + 64 * s + 16 * half),
                                            *reinterpret_cast<const i32x4_t*>(qr + 64 * s + 32 + 16 * half), 0, 1, 2, 3, 4, 5, 6, 7);
        const unsigned w = *reinterpret_cast<const unsigned*>(qs + (int64_t)qrow * p.q_sld);
#pragma unroll
        for (int s = 0; s < 2; ++s) qsc[s] = (int)__builtin_amdgcn_ubfe(w, (unsigned)(16 * s + 8 * half), 8u);
        // retire the loads here, not at the first use inside the key loop (attention.hip: the counted waits would cover the tile DMA too)
#pragma unroll
        for (int s = 0; s < 2; ++s) asm volatile("" : "+v"(qf[s]), "+v"(qsc[s]));
    }

    // ---- DMA staging: wave w moves pieces w and w + 4 of the K tile (8 rows of 128 B each) and of the V^T tile (16 rows of 64 B each)
    const int kr0 = 8 * wave + (lane >> 3);                                   // K row of piece j: kr0 + 32 j
    const int kch = ((lane & 7) ^ kswz(kr0)) * 16;                            // (kswz(kr0 + 32) == kswz(kr0))
    const int vr0 = 16 * wave + (lane >> 2);                                  // V^T row of piece j: vr0 + 64 j
    const unsigned vvoff = (unsigned)(vr0 * p.vt_ld + ((lane & 3) ^ vswz(vr0)) * 16);
    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;
    // K rows of the last tile that lie past Lk are clamped to Lk - 1 (a real row; their scores are masked): only when `clamp` (wave-uniform)
    // does a lane compute its own row, otherwise the tile offset is in the SGPR base and the lane offsets are fixed
    const unsigned kvoff0 = (unsigned)(kr0 * p.k_ld + kch), kvoff1 = (unsigned)((kr0 + 32) * p.k_ld + kch);
    auto issue_tile = [&](const int kt, const int buf, const bool clamp) {
        const unsigned dst = lds_base + buf * STAGE + wave * 1024;
        if (clamp) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int r = kt * KT + kr0 + 32 * j;
                if (r > Lk - 1) r = Lk - 1;
                glds16_fa((unsigned)(r * p.k_ld + kch), kp, __builtin_amdgcn_readfirstlane(dst + j * 4096));
            }
        } else {
            const unsigned char* kb = kp + (int64_t)kt * KT * p.k_ld;
            glds16_fa(kvoff0, kb, __builtin_amdgcn_readfirstlane(dst));
            glds16_fa(kvoff1, kb, __builtin_amdgcn_readfirstlane(dst + 4096));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
            glds16_fa(vvoff, vp + (int64_t)kt * KT + (int64_t)j * 64 * p.vt_ld, __builtin_amdgcn_readfirstlane(dst + K_BYTES + j * 4096));
    };
    // scales of a tile, straight from global memory into registers one tile ahead: the K rows' dwords (score block sb) and the V^T rows'
    // two blocks of the tile (channel block db); uniform bases + fixed 32-bit lane offsets, K rows clamped as above
    const int prow = (l31 & 3) | ((l31 >> 3) << 2) | (((l31 >> 2) & 1) << 4);        // pi(l31)
    const unsigned ksoff[2] = {(unsigned)(prow * p.k_sld), (unsigned)((prow + 32) * p.k_sld)};
    unsigned vsoff[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) vsoff[db] = (unsigned)((32 * db + l31) * p.vt_sld);
    unsigned ksw[2], vsw[4];
    auto load_scales = [&](const int kt, const bool clamp) {
        if (clamp) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                int r = kt * KT + 32 * sb + prow;
                if (r > Lk - 1) r = Lk - 1;
                ksw[sb] = *reinterpret_cast<const unsigned*>(ks + (unsigned)(r * p.k_sld));
            }
        } else {
            const unsigned char* kb = ks + (int64_t)kt * KT * p.k_sld;
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) ksw[sb] = *reinterpret_cast<const unsigned*>(kb + ksoff[sb]);
        }
        const unsigned char* vb = vs + 2 * kt;
#pragma unroll
        for (int db = 0; db < 4; ++db) vsw[db] = *reinterpret_cast<const unsigned short*>(vb + vsoff[db]);
    };

    // fragment read offsets inside a stage: K row pi(l31) (+ 32 rows per score block), slots 4s + h and 4s + 2 + h; V^T row l31 (+ 32 rows
    // per channel block), slots h and 2 + h
    unsigned koff[2][2], voff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 2; ++e) koff[s][e] = (unsigned)(prow * 128 + (((4 * s + 2 * e + half) ^ kswz(prow)) << 4));
#pragma unroll
    for (int e = 0; e < 2; ++e) voff[e] = (unsigned)(l31 * 64 + (((2 * e + half) ^ vswz(l31)) << 4));
    auto ld8 = [&](const unsigned char* base, const unsigned lo, const unsigned hi) {
        return __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(base + lo), *reinterpret_cast<const i32x4_t*>(base + hi), 0, 1, 2, 3, 4, 5, 6, 7);
    };

    // O^T and the row sums (an all-ones A operand against P^T: l_j in every register of query j's lanes, from the same fp32 accumulation as O,
    // on the matrix pipe, which has room - the VALU has none)
    f32x16_t o[4], lacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i][r] = 0.0f;
        lacc[r] = 0.0f;
    }
    float m_run = -INFINITY;
    const float sc = p.scale * 1.4426950408889634f;   // softmax in base 2
    const float pexp = (float)(8 - DEFER);             // P 2^(8 - DEFER): codes in [0, 256]
    constexpr int pscale = P_SCALE + DEFER;
    const i32x8_t ones = {0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};
    const int nfull = Lk / KT;                         // whole tiles; a partial last tile runs the masked body once after the loop

    // one 64-key tile; TAIL: the partial last tile (keys >= Lk masked)
    auto tile_body = [&](const int kt, auto TAIL_c) {
        constexpr bool TAIL = decltype(TAIL_c)::value;
        const int buf = kt & 1;
        // tile kt (and its scales) has landed; every fragment read of tile kt - 1 has returned, so its stage may be overwritten
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // this tile's scale bytes, taken out before the next tile's loads are issued: K block 2s + half of score block sb, V^T block 2kt + half
        int ksc[2][2], vsc[4];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int s = 0; s < 2; ++s) ksc[sb][s] = (int)__builtin_amdgcn_ubfe(ksw[sb], (unsigned)(16 * s + 8 * half), 8u);
#pragma unroll
        for (int db = 0; db < 4; ++db) vsc[db] = (int)__builtin_amdgcn_ubfe(vsw[db], (unsigned)(8 * half), 8u);
        if constexpr (TAIL) {
            if (kt * KT + 32 * half >= Lk) {                                 // a V^T block wholly past Lk: its byte may be anything
#pragma unroll
                for (int db = 0; db < 4; ++db) vsc[db] = 127;
            }
        }
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) asm volatile("" : "+v"(ksc[sb][0]), "+v"(ksc[sb][1]));
#pragma unroll
        for (int db = 0; db < 4; ++db) asm volatile("" : "+v"(vsc[db]));
        if (!TAIL && kt + 1 < ntiles) {
            const bool clamp = (kt + 2) * KT > Lk;
            issue_tile(kt + 1, buf ^ 1, clamp);
            load_scales(kt + 1, clamp);
        }
        const unsigned char* Ks = lds + buf * STAGE;
        const unsigned char* Vs = Ks + K_BYTES;

        // S^T = K Q^T: every K fragment of the tile requested before the first MFMA
        i32x8_t kf[2][2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int s = 0; s < 2; ++s) kf[sb][s] = ld8(Ks + sb * 32 * 128, koff[s][0], koff[s][1]);
        __builtin_amdgcn_sched_barrier(0);
        f32x16_t sacc[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[sb][r] = 0.0f;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int s = 0; s < 2; ++s) sacc[sb] = mfma_mx8(kf[sb][s], qf[s], sacc[sb], ksc[sb][s], qsc[s]);
        __builtin_amdgcn_s_setprio(0);
        // ... and the V^T fragments before the softmax, whose VALU work covers their latency
        i32x8_t vf[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) vf[db] = ld8(Vs + db * 32 * 64, voff[0], voff[1]);
        __builtin_amdgcn_sched_barrier(0);

        // online softmax, base 2 (attn_kernel's): C register r of lane half h = key kt 64 + 32 sb + 16 h + r
        float mt = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (TAIL) {
                    if (kt * KT + 32 * sb + 16 * half + r >= Lk) sacc[sb][r] = -INFINITY;
                }
                mt = fmaxf(mt, sacc[sb][r]);
            }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);
        if (__any((m_new - m_run) * sc > (float)DEFER)) {                       // m_run = -inf on the first tile -> inf > DEFER
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);    // ... and alpha = 0
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i][r] *= alpha;
                lacc[r] *= alpha;
            }
            m_run = m_new;
        }
        const float neg_m = fmaf(-m_run, sc, pexp);
        // P^T operand: codes e4m3(P 2^(8 - DEFER)) of score block sb in registers 4 sb .. 4 sb + 3 (the first conversion's old value is
        // overwritten by the second: no zeroing move)
        i32x8_t pf;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float e[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) e[i] = __builtin_amdgcn_exp2f(fmaf(sacc[sb][4 * w + i], sc, neg_m));
                int v = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], __builtin_bit_cast(int, e[0]), false);
                v = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], v, true);
                pf[4 * sb + w] = v;
            }
        if constexpr (TAIL) {
            // V^T codes of keys >= Lk (register g of lane half h: keys kt 64 + 32 (g >> 2) + 16 h + 4 (g & 3) .. + 3) become zeros
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const int nv = Lk - (kt * KT + 32 * (g >> 2) + 16 * half + 4 * (g & 3));
                const unsigned m = nv >= 4 ? 0xffffffffu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u));
#pragma unroll
                for (int db = 0; db < 4; ++db) vf[db][g] = (int)((unsigned)vf[db][g] & m);
            }
        }

        // O^T += V^T P^T, l += 1 P^T
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int db = 0; db < 4; ++db) o[db] = mfma_mx8(vf[db], pf, o[db], vsc[db], pscale);
        lacc = mfma_mx8(ones, pf, lacc, 127, pscale);
        __builtin_amdgcn_s_setprio(0);
    };

    issue_tile(0, 0, KT > Lk);
    load_scales(0, KT > Lk);
    for (int kt = 0; kt < nfull; ++kt) tile_body(kt, std::false_type{});
    if (nfull < ntiles) tile_body(nfull, std::true_type{});

    // O / l: both in dequantised units (a constant V comes out as itself)
    const float inv = 1.0f / lacc[0];
    const int qrow = q0 + l31;
    if (qrow < p.Lq) {
        bf16_t* op = (bf16_t*)p.o + (int64_t)b * p.o_bstride + (int64_t)qrow * p.o_ld + h * D + 4 * half;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2_t w;
                w[0] = pack2<bf16_t>(o[db][4 * g] * inv, o[db][4 * g + 1] * inv);
                w[1] = pack2<bf16_t>(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
                *reinterpret_cast<u32x2_t*>(op + 32 * db + 8 * g) = w;
            }
    }
}

}  // namespace

namespace omgsr {
// omgsr_attention with qkv_el = OMGSR_EL_MXFP8 (the caller has checked the common fields)
int mxfp8_attention(const omgsr_attn_args& a, hipStream_t st) {
    if (a.D != D || (a.vt_ld % 128) || a.vt_ld < a.Lk || (a.q_ld & 15) || (a.k_ld & 15) || (a.o_ld & 3) || compute_dtype() != 0) return OMGSR_E_SHAPE;
    if (a.o_lo_off || a.o_mx || a.q_lo_off || a.k_lo_off || a.p_split || a.vt_lo_off || a.qkv_reserved) return OMGSR_E_SHAPE;
    if (!a.q_scale || !a.k_scale || !a.vt_scale) return OMGSR_E_BADARG;
    const auto mis = [](const void* ptr, const int m) { return ((size_t)ptr & (size_t)(m - 1)) != 0; };
    if (mis(a.q, 16) || mis(a.k, 16) || mis(a.vt, 16) || (a.q_bstride & 15) || (a.k_bstride & 15) || (a.vt_bstride & 15)) return OMGSR_E_SHAPE;
    if (mis(a.q_scale, 4) || mis(a.k_scale, 4) || mis(a.vt_scale, 2) || (a.q_sld & 3) || (a.k_sld & 3) || (a.vt_sld & 1) ||
        (a.q_sbstride & 3) || (a.k_sbstride & 3) || (a.vt_sbstride & 1) || a.q_sld < a.H * 4 || a.k_sld < a.H * 4 || a.vt_sld < a.vt_ld / 32)
        return OMGSR_E_SHAPE;
    // 32-bit DMA offsets: (Lk - 1) k_ld + 128 and 127 vt_ld + 64 from the SGPR bases
    if ((int64_t)a.Lk * a.k_ld >= (1ll << 31) || 128ll * a.vt_ld >= (1ll << 31)) return OMGSR_E_SHAPE;
    const int ntiles = (a.Lk + KT - 1) / KT;
    const int qtiles = (a.Lq + 127) / 128;
    const int64_t blocks = (int64_t)qtiles * a.H * a.B;
    if (blocks > 0x7fffffffll) return OMGSR_E_SHAPE;
    const double flops = 4.0 * (double)a.B * a.H * (double)a.Lq * a.Lk * a.D;
    const double bytes = (double)a.B * a.H * a.D * (33.0 / 32.0 * (a.Lq + 2.0 * a.Lk) + 2.0 * a.Lq);
    TimingScope ts(OMGSR_TK_ATTN, flops, bytes, st, (long long)a.B * a.H * a.Lq, a.Lk, a.D);
    if (ts.active) ts.rec.variant = 19;
    return launch_lds<mxfp8_attn_kernel>(dim3((unsigned)blocks), dim3(256), LDS_BYTES, st, a, ntiles, qtiles);
}
}  // namespace omgsr
