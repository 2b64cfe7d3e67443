// Fused attention softmax(Q K^T * scale) V at head_dim 512 for gfx950: the VAE mid block's one-head attention (omgsr_attention with D = 512,
// timing variant 20). Same orientation as attn_kernel (attention.hip): S^T = K Q^T and O^T = V^T P^T with v_mfma_f32_32x32x16, one query per
// lane pair, the P^T operand converted in place from the score registers (contraction slot j of half h <-> key (j&3) + 8*(j>>2) + 4h of a
// 16-key group, matched on the V^T side by two 8-byte reads).
//
// What D = 512 changes:
//  * a wave's 32 queries need 128 registers of Q fragments, and the whole O^T would be 256 accumulator registers on top: the output channels
//    are split over NPART = 512 / NCH workgroups (consecutive block ids, so the parts of a query tile run side by side on one XCD and share
//    its L2). Each part computes the full scores and NCH channels of O^T: 128 (NCH = 256) accumulator registers, one wave per SIMD.
//    The two-term-split form (q_lo_off / k_lo_off, accurate tier) holds Q_lo as well (256 registers of Q) and takes NCH = 128.
//  * key tiles of 32: a K tile is 32 KB (64 KB with K_lo), a V^T part 16 KB; two stages fit the 160 KB of LDS.
//  * K rows are exactly one LDS-DMA piece (1 KiB = 64 lanes x 16 B): wave w moves rows w, w + 4, ... with `global_load_lds_dwordx4`, the row
//    address in SGPRs (64-bit, clamped to the last valid key: a partial last tile re-reads row Lk - 1 and its scores are masked), the
//    16-byte chunk XOR-swizzled with the row on the SOURCE side (slot i of row r holds chunk i ^ (r & 15): conflict-free ds_read_b128).
//  * V^T goes through registers (16-byte loads, masked past Lk so that padding never reaches an MFMA: 0 * NaN), rows padded to 72 B
//    (18 banks: conflict-free ds_read_b64); it is loaded at the top of a tile and written to the other stage after the tile's MFMAs.
//  * one barrier per tile.
//
// FULL (vae_attn_full_kernel, timing variant 23: the range-fallback tier, omgsr_attn_args.p_split with vt_lo_off): every operand a two-term
// split. On top of the split q / k, V^T_lo (vp + vt_lo_off) is staged next to V^T_hi with the same pitch and the same masking, the probabilities
// are split in place from the fp32 score registers (p_hi = (T)e, p_lo = (T)(e - p_hi), the row sum from the fp32 e), and a channel block runs
// three PV passes, the two correction products first: O^T += V_hi^T P_lo^T + V_lo^T P_hi^T + V_hi^T P_hi^T. NCH = 64 (8 parts per query tile):
// two stages of [K_hi | K_lo | V^T_hi | V^T_lo] are 2 (65536 + 2 * 64 * 72) = 149504 B; NCH = 128 would need 167936 B.
#include "common.hip.h"
#include "../../include/omgsr_hip.h"
#include "timing.hip.h"

namespace {

constexpr int D = 512, KT = 32;                 // head_dim, keys per tile
constexpr int K_BYTES = KT * 2 * D;             // one K tile (unpadded, swizzled)
constexpr int VP = 72;                          // V^T row pitch in bytes (64 of data)

OMGSR_DEVINL void glds16_row(const unsigned voff, const void* sbase, const unsigned lds_dst) {
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

template <typename T, int NCH, bool SPLIT, bool FULL>
OMGSR_DEVINL void vae_attn_body(const omgsr_attn_args& p, const int ntiles, const float defer, const int qtiles, const int xcd_order) {
    static_assert(SPLIT || !FULL, "split P / V^T come with split q / k");
    constexpr int NPART = D / NCH;
    constexpr int KT_BYTES = SPLIT ? 2 * K_BYTES : K_BYTES;          // [K_hi | K_lo] of a tile
    constexpr int V_BYTES = NCH * VP;
    constexpr int STAGE = KT_BYTES + (FULL ? 2 * V_BYTES : V_BYTES);  // ... then [V^T_hi | V^T_lo]
    constexpr int NVC = NCH * 4 / 256;          // 16-byte V^T chunks per thread
    constexpr int NKS = D / 16, NDB = NCH / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    // 1-D grid of NPART x qtiles x H x B workgroups, the parts of a query tile innermost; xcd_remap gives each XCD a contiguous range, so the
    // query tiles of an image sweep its K / V^T (2 MB per 1024 keys) through ONE L2 together
    const int tile = xcd_order ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int part = tile % NPART, qt = (tile / NPART) % qtiles, bh = tile / (NPART * qtiles);
    const int h = bh % p.H, b = bh / p.H;
    const int q0 = qt * 128 + wave * 32;

    const T* __restrict__ qp = (const T*)p.q + (int64_t)b * p.q_bstride + h * D;
    const T* __restrict__ kp = (const T*)p.k + (int64_t)b * p.k_bstride + h * D;
    const T* __restrict__ vp = (const T*)p.vt + (int64_t)b * p.vt_bstride + ((int64_t)h * D + part * NCH) * p.vt_ld;

    // Q^T operand fragments live in registers for the whole sweep
    x8_t<T> qf[NKS], qfl[SPLIT ? NKS : 1];
    {
        int qrow = q0 + l31; if (qrow > p.Lq - 1) qrow = p.Lq - 1;
        const T* qr = qp + (int64_t)qrow * p.q_ld + 8 * half;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const x8_t<T>*>(qr + 16 * ks);
        if constexpr (SPLIT) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) qfl[ks] = *reinterpret_cast<const x8_t<T>*>(qr + p.q_lo_off + 16 * ks);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qfl[ks]));
        }
        // retire the loads here, not at their first use inside the key loop (where the wait would also cover the next tile's DMA)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[ks]));
    }

    typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
    const unsigned lds_base = (unsigned)(size_t)(lds_byte_t*)lds;
    // K tile kt -> stage buf: row r = 4 j + wave of the tile is one piece; lane i fetches chunk i ^ (r & 15)
    auto issue_k = [&](const int kt, const int buf) {
#pragma unroll
        for (int j = 0; j < KT / 4; ++j) {
            const int r = 4 * j + wave;
            int key = kt * KT + r; if (key > p.Lk - 1) key = p.Lk - 1;
            const unsigned voff = (unsigned)((lane ^ (r & 15)) << 4);
            const unsigned char* src = reinterpret_cast<const unsigned char*>(kp + (int64_t)key * p.k_ld);
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + buf * STAGE + r * 2 * D);
            glds16_row(voff, src, dst);
            if constexpr (SPLIT) glds16_row(voff, src + (int64_t)p.k_lo_off * 2, __builtin_amdgcn_readfirstlane(dst + K_BYTES));
        }
    };
    u32x4_t vreg[NVC], vregl[FULL ? NVC : 1];
    // eight keys of a V^T row, zero past Lk
    auto load_v8 = [&](const T* src, const int nvalid) {
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (nvalid > 0) {
            v = *reinterpret_cast<const u32x4_t*>(src);
            if (nvalid < 8) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (2 * w >= nvalid) v[w] = 0u;
                    else if (2 * w + 1 >= nvalid) v[w] &= 0xffffu;
                }
            }
        }
        return v;
    };
    auto load_v = [&](const int kt) {
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int c = t + 256 * i;
            const int drow = c >> 2, kc = c & 3;
            const int key0 = kt * KT + kc * 8;
            const T* src = vp + (int64_t)drow * p.vt_ld + key0;
            vreg[i] = load_v8(src, p.Lk - key0);
            if constexpr (FULL) vregl[i] = load_v8(src + p.vt_lo_off, p.Lk - key0);
        }
    };
    auto write_v = [&](const int buf) {
        unsigned char* Vs = lds + buf * STAGE + KT_BYTES;
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int c = t + 256 * i;
            unsigned char* d = Vs + (c >> 2) * VP + (c & 3) * 16;      // 8-byte aligned only
            *reinterpret_cast<u32x2_t*>(d) = (u32x2_t){vreg[i][0], vreg[i][1]};
            *reinterpret_cast<u32x2_t*>(d + 8) = (u32x2_t){vreg[i][2], vreg[i][3]};
            if constexpr (FULL) {
                *reinterpret_cast<u32x2_t*>(d + V_BYTES) = (u32x2_t){vregl[i][0], vregl[i][1]};
                *reinterpret_cast<u32x2_t*>(d + V_BYTES + 8) = (u32x2_t){vregl[i][2], vregl[i][3]};
            }
        }
    };

    f32x16_t o[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float sc = p.scale * 1.4426950408889634f;   // softmax in base 2

    // K fragment of contraction step ks: row l31, chunk 2 ks + half at slot chunk ^ (row & 15). The XOR touches the low four bits of the
    // chunk index only, so eight per-lane offsets (ks & 7) serve the row; 256 (ks >> 3) is an immediate
    unsigned koff[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) koff[i] = (unsigned)(l31 * 2 * D + (((2 * i + half) ^ (l31 & 15)) << 4));

    issue_k(0, 0);
    load_v(0);
    write_v(0);

    for (int kt = 0; kt < ntiles; ++kt) {
        const int buf = kt & 1;
        // tile kt has landed (this wave's K pieces and V^T writes; the barrier extends that to every wave's) and every fragment read of
        // tile kt - 1 has returned, so its stage may be overwritten
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool more = kt + 1 < ntiles;
        if (more) {
            issue_k(kt + 1, buf ^ 1);
            load_v(kt + 1);
        }
        const unsigned char* Ks = lds + buf * STAGE;
        const unsigned char* Vs = Ks + KT_BYTES;

        // S^T = K Q^T: one 32-key block
        f32x16_t s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
        if constexpr (SPLIT) {          // the two correction products first (small terms into the empty accumulator), then the main product
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const x8_t<T> kl = *reinterpret_cast<const x8_t<T>*>(Ks + K_BYTES + koff[ks & 7] + 256 * (ks >> 3));
                s = mfma32(kl, qf[ks], s);
                if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);         // at most 8 K fragments in flight (32 registers)
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const x8_t<T> kf = *reinterpret_cast<const x8_t<T>*>(Ks + koff[ks & 7] + 256 * (ks >> 3));
                s = mfma32(kf, qfl[ks], s);
                if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);         // at most 8 K fragments in flight (32 registers)
            }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const x8_t<T> kf = *reinterpret_cast<const x8_t<T>*>(Ks + koff[ks & 7] + 256 * (ks >> 3));
            s = mfma32(kf, qf[ks], s);
                if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);         // at most 8 K fragments in flight (32 registers)
        }

        // online softmax (one query per lane pair), base 2, exactly as attn_kernel: raw scores, p = exp2(fma(s, sc, -m sc)); the running
        // maximum (and with it O and l, all of which are still at the old maximum: nothing of this tile has been accumulated yet) moves only
        // when some row of the wave saw its maximum grow by more than 2^defer (omgsr_set_attention_defer_max; 0 = exact running maximum)
        const bool tail = (kt == ntiles - 1) && (p.Lk & (KT - 1));
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (tail && (kt * KT + cfrag_row(lane, r) >= p.Lk)) s[r] = -INFINITY;
            mt = fmaxf(mt, s[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);
        if (__any((m_new - m_run) * sc > defer)) {                                // m_run = -inf on the first tile -> inf > defer
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);    // ... and alpha = 0
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < NDB; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            m_run = m_new;
        }
        const float neg_m = -m_run * sc;
        float rs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[r], sc, neg_m));
            s[r] = e;
            rs += e;
        }
        l_run += rs;

        // P^T operand: score registers converted in place (key permutation, see header)
        x8_t<T> pf[2], pfl[FULL ? 2 : 1];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[u][j] = (T)s[8 * u + j];
        if constexpr (FULL) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) pfl[u][j] = (T)(s[8 * u + j] - (float)pf[u][j]);
        }

        // O^T += V^T P^T
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const unsigned char* vr = Vs + (32 * db + l31) * VP + 8 * half;
            // the 16 keys of half-tile u of this lane's channel row: two 8-byte reads (key permutation, see header)
            auto v_frag = [&](const unsigned char* a) {
                const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(a);
                const u32x2_t hi = *reinterpret_cast<const u32x2_t*>(a + 16);
                const u32x4_t both = {lo[0], lo[1], hi[0], hi[1]};
                return __builtin_bit_cast(x8_t<T>, both);
            };
            if constexpr (FULL) {       // the two correction products first, as in the score passes
                const x8_t<T> vh[2] = {v_frag(vr), v_frag(vr + 32)}, vl[2] = {v_frag(vr + V_BYTES), v_frag(vr + V_BYTES + 32)};
#pragma unroll
                for (int u = 0; u < 2; ++u) o[db] = mfma32(vh[u], pfl[u], o[db]);
#pragma unroll
                for (int u = 0; u < 2; ++u) o[db] = mfma32(vl[u], pf[u], o[db]);
#pragma unroll
                for (int u = 0; u < 2; ++u) o[db] = mfma32(vh[u], pf[u], o[db]);
            } else {
#pragma unroll
                for (int u = 0; u < 2; ++u) o[db] = mfma32(v_frag(vr + 32 * u), pf[u], o[db]);
            }
        }
        if (more) write_v(buf ^ 1);
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    const int qrow = q0 + l31;
    if (qrow < p.Lq) {
        T* op = (T*)p.o + (int64_t)b * p.o_bstride + (int64_t)qrow * p.o_ld + h * D + part * NCH + 4 * half;
        const int lo_off = p.o_lo_off;       // > 0: the low halves of the two-term split land that many columns later
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v0 = o[db][4 * g] * inv, v1 = o[db][4 * g + 1] * inv, v2 = o[db][4 * g + 2] * inv, v3 = o[db][4 * g + 3] * inv;
                u32x2_t w;
                w[0] = pack2<T>(v0, v1);
                w[1] = pack2<T>(v2, v3);
                *reinterpret_cast<u32x2_t*>(op + 32 * db + 8 * g) = w;
                if (lo_off > 0) {
                    u32x2_t l;
                    l[0] = pack2<T>(v0 - lo_of<T>(w[0], 0), v1 - lo_of<T>(w[0], 1));
                    l[1] = pack2<T>(v2 - lo_of<T>(w[1], 0), v3 - lo_of<T>(w[1], 1));
                    *reinterpret_cast<u32x2_t*>(op + lo_off + 32 * db + 8 * g) = l;
                }
            }
    }
}

// <compute type, channels per workgroup, two-term-split q / k>
template <typename T, int NCH, bool SPLIT>
__global__ __launch_bounds__(256, 1) void vae_attn_kernel(const omgsr_attn_args p, const int ntiles, const float defer, const int qtiles, const int xcd_order) {
    vae_attn_body<T, NCH, SPLIT, false>(p, ntiles, defer, qtiles, xcd_order);
}

// every operand a two-term split (FULL)
template <typename T, int NCH>
__global__ __launch_bounds__(256, 1) void vae_attn_full_kernel(const omgsr_attn_args p, const int ntiles, const float defer, const int qtiles, const int xcd_order) {
    vae_attn_body<T, NCH, true, true>(p, ntiles, defer, qtiles, xcd_order);
}

template <typename T, int NCH, bool SPLIT, bool FULL>
constexpr auto vae_attn_fn() {
    if constexpr (FULL) return &vae_attn_full_kernel<T, NCH>;
    else return &vae_attn_kernel<T, NCH, SPLIT>;
}

template <int NCH, bool SPLIT, bool FULL = false>
int launch_vae_attn(const omgsr_attn_args& a, hipStream_t st, const float defer) {
    constexpr int LDS = 2 * ((SPLIT ? 2 : 1) * K_BYTES + (FULL ? 2 : 1) * NCH * VP);
    static_assert(LDS <= 160 * 1024, "two stages must fit the LDS");
    // every choice below depends on one sample's Lq / Lk only (batch-invariant by construction)
    const int ntiles = (a.Lk + KT - 1) / KT;
    const int qtiles = (a.Lq + 127) / 128;
    const int64_t blocks = (int64_t)qtiles * (D / NCH) * a.H * a.B;
    if (blocks > 0x7fffffffll) return OMGSR_E_SHAPE;
    static const char* xo = getenv("OMGSR_ATTN_XCD");            // A/B runs: "0" = natural block order
    const int xcd_order = !(xo && xo[0] == '0');
    OMGSR_DISPATCH_T(return launch_lds<vae_attn_fn<T, NCH, SPLIT, FULL>()>(dim3((unsigned)blocks), dim3(256), LDS, st, a, ntiles, defer, qtiles, xcd_order));
}

}  // namespace

namespace omgsr {
// omgsr_attention with D = 512 and 16-bit operands (the caller has checked the pointers, the leading dimensions' alignment and o_lo_off)
int vae_attention(const omgsr_attn_args& a, hipStream_t st, const float defer) {
    // plain or two-term-split q / k, single or two-term-split output; split P and split V^T come together and with split q / k (the
    // range-fallback tier's form: vae_attn_full_kernel); no MX output at this head size
    if (a.o_mx) return OMGSR_E_SHAPE;
    const bool split = a.q_lo_off != 0 || a.k_lo_off != 0;
    if (split && (a.q_lo_off <= 0 || a.k_lo_off <= 0 || (a.q_lo_off & 7) || (a.k_lo_off & 7))) return OMGSR_E_SHAPE;
    const bool full = a.p_split != 0 || a.vt_lo_off != 0;
    if (full && (!split || !a.p_split || a.vt_lo_off <= 0 || (a.vt_lo_off & 7))) return OMGSR_E_SHAPE;
    const auto mis = [](const void* ptr) { return ((size_t)ptr & 15) != 0; };
    if (mis(a.q) || mis(a.k) || mis(a.vt) || ((size_t)a.o & 7) || (a.q_bstride & 7) || (a.k_bstride & 7) || (a.vt_bstride & 7) || (a.o_bstride & 3)) return OMGSR_E_SHAPE;
    const double flops = 4.0 * (double)a.B * a.H * (double)a.Lq * a.Lk * a.D;
    const double bytes = 2.0 * (double)a.B * a.H * a.D * ((split ? 3.0 : 2.0) * a.Lq + (full ? 4.0 : split ? 3.0 : 2.0) * a.Lk);
    TimingScope ts(OMGSR_TK_ATTN, flops, bytes, st, (long long)a.B * a.H * a.Lq, a.Lk, a.D);
    if (ts.active) ts.rec.variant = full ? 23 : 20;
    if (full) return launch_vae_attn<64, true, true>(a, st, defer);
    return split ? launch_vae_attn<128, true>(a, st, defer) : launch_vae_attn<256, false>(a, st, defer);
}
}  // namespace omgsr
