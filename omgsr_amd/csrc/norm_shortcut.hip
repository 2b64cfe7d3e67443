// norm1's GroupNorm apply pass of a ResnetBlock whose channel count changes, with the block's 1x1 conv_shortcut computed in the same pass
// (accurate tier, fp32 stream tensor, fp16 compute type): x crosses HBM once instead of three times (apply read, cast-twin write, twin re-read
// by the shortcut GEMM). (Timing: kind 1, variant 29.)
//
// gn_shortcut_kernel<PT, NTW, YEL> (omgsr_groupnorm_shortcut): a workgroup owns P = 32 PT consecutive pixels of one row (image or tile) and all
//   N = 128 NTW shortcut outputs, and walks C in chunks of 64 channels. Per chunk:
//     * thread t loads octet (t & 7) of pixels (t >> 3) + 32 i from the fp32 map - the apply body's lane mapping: consecutive lanes hold
//       consecutive octets of a pixel, so the cooperative store8_mx6 works;
//     * y gets exactly the arithmetic of gn_apply_any_body: the (scale, shift) table of the row's image in LDS, v = x a + (beta - mean a),
//       silu_f, then store8 / store8_mx6 - the bytes of the apply pass;
//     * the RAW octet is split into fp16 hi / lo (split8) and written to an LDS tile [pixel][octet] (rows of 9 x 16 bytes: the 32 rows a
//       fragment read touches fall on different banks);
//     * wave w multiplies the whole pixel tile by output columns [32 NTW w, 32 NTW (w + 1)): per 16-channel step and 32 x 32 tile, three
//       v_mfma_f32_32x32x16_f16 in the fixed order x_hi w_hi, x_lo w_hi, x_hi w_lo into one fp32 accumulator. The weight fragments come
//       straight from global memory (L2): the packed weight is [chunk][step][column tile][hi | lo][lane][8 fp16], a wave's load is 1 KB
//       contiguous. The next chunk's x loads are issued before the MFMAs.
//   The summation order is (chunk, step, segment), independent of the grid: two launches, or the multi launch and a launch per group, give
//   the same bits. At the end each 32 x 32 accumulator tile goes through a wave-private LDS transpose and leaves as 16-byte row stores with the
//   bias added. Pixels past the row's end are loaded as zeros and never stored.
//   Several tensors of one layer (the tiled VAE's tile-shape groups) share a launch through a prefix table of workgroup counts, the way
//   gn_apply_any_multi_kernel does it.
//   Pixel tile: P = 128 at N = 128, 96 at N = 256, 64 at N = 512 (64, 96, 128 accumulator registers).
//   LDS: tile 2 x P x 144 B (hi, lo) + the 4 KB table: 40 KB at P = 128, 31 KB at 96, 22 KB at 64; two workgroups per CU by registers (<= 256).
#include "common.hip.h"
#include "timing.hip.h"
#include "../../include/omgsr_hip.h"

namespace {

constexpr int GS_CK = 64;             // channels per chunk
constexpr int GS_ROW = 9;             // 16-byte units per LDS tile row (8 octets + 1 pad)
constexpr int GS_MAXC = 512;
constexpr int GS_EP_LD = 36;          // floats per row of the epilogue's 32 x 32 transpose tile (32 + 4 pad: 16-byte aligned rows)

struct GnShortcutTable {
    const float* x[OMGSR_GN_MAX_GROUPS];
    void* y[OMGSR_GN_MAX_GROUPS];
    float* sc[OMGSR_GN_MAX_GROUPS];
    int HW[OMGSR_GN_MAX_GROUPS];
    int tiles[OMGSR_GN_MAX_GROUPS];                        // pixel tiles per tensor row (image or tile)
    int start[OMGSR_GN_MAX_GROUPS + 1];                    // first workgroup of group k; start[count] = grid size
    int count;
};

template <int PT, int NTW, int YEL>
__global__ __launch_bounds__(256, 2) void gn_shortcut_kernel(const GnShortcutTable m, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const u32x4_t* __restrict__ wpk, const float* __restrict__ bias,
                                                              const int C, const int G, const int act, const int stat_rows,
                                                              unsigned* __restrict__ ovf) {
    using T = f16_t;
    constexpr int P = 32 * PT, NT = 4 * NTW, N = 32 * NT;
    static_assert(2 * P * GS_ROW * 16 >= 4 * 32 * GS_EP_LD * 4, "the epilogue's four transpose tiles reuse the operand tile");
    __shared__ __attribute__((aligned(16))) u32x4_t tile[2 * P * GS_ROW];      // [hi | lo][pixel][GS_ROW]
    __shared__ __attribute__((aligned(16))) float tab[2 * GS_MAXC];            // scale [C] | shift [C]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int s = 0;
    while (s + 1 < m.count && (int)blockIdx.x >= m.start[s + 1]) ++s;          // wave-uniform
    const int local = (int)blockIdx.x - m.start[s];
    const int n = local / m.tiles[s];
    const int HW = m.HW[s];
    const int p0 = (local - n * m.tiles[s]) * P;
    const float* __restrict__ x = m.x[s];
    void* __restrict__ y = m.y[s];
    float* __restrict__ scout = m.sc[s];

    // the (scale, shift) table of this row's image: the two expressions of the apply kernels
    float* sc = tab;
    float* sh = tab + C;
    const int ns = n % stat_rows;          // tiled VAE: rows are (tile, image) tile-major and share the image's statistics
    const int cpg = C / G;
    for (int c = t; c < C; c += 256) {
        const int g = c / cpg;
        const float r = rstd[ns * G + g], mu = mean[ns * G + g];
        const float a = r * (gamma ? gamma[c] : 1.0f);
        sc[c] = a;
        sh[c] = (beta ? beta[c] : 0.0f) - mu * a;
    }
    __syncthreads();
    auto transform = [&](float (&f)[8], const int cc) {
        const f32x4_t* sa = reinterpret_cast<const f32x4_t*>(sc + cc * 8);
        const f32x4_t* ha = reinterpret_cast<const f32x4_t*>(sh + cc * 8);
        const f32x4_t sa0 = sa[0], sa1 = sa[1], ha0 = ha[0], ha1 = ha[1];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = f[e] * (e < 4 ? sa0[e & 3] : sa1[e & 3]) + (e < 4 ? ha0[e & 3] : ha1[e & 3]);
            f[e] = (act == OMGSR_ACT_SILU) ? silu_f(v) : v;
        }
    };

    const int oct = t & 7, prow = t >> 3;          // this thread's octet of the chunk and its pixel of every 32-pixel pass
    const int64_t pix0 = (int64_t)n * HW + p0;     // first pixel of the tile in the tensor
    float raw[PT][8];
    auto fetch = [&](const int chunk) {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            if (p0 + prow + 32 * i < HW) load8<T, true>(x, (pix0 + prow + 32 * i) * C + chunk * GS_CK + oct * 8, raw[i]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) raw[i][e] = 0.0f;
            }
        }
    };

    f32x16_t acc[PT][NTW];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float amax = 0.0f;          // fp16 range guard of the raw operand (see omgsr_igemm_args.overflow_flag)

    u32x4_t* thi = tile;
    u32x4_t* tlo = tile + P * GS_ROW;
    const int arow = (lane & 31) * GS_ROW + (lane >> 5);      // A fragment: row lane & 31, k = 8 (lane >> 5) + j
    const int nchunk = C / GS_CK;
    fetch(0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            u32x4_t hi, lo;
            split8<T>(raw[i], hi, lo);
            thi[(prow + 32 * i) * GS_ROW + oct] = hi;
            tlo[(prow + 32 * i) * GS_ROW + oct] = lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(raw[i][e]));
        }
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const bool valid = p0 + prow + 32 * i < HW;          // the same for the eight lanes of a pixel, so for every lane quad
            const int64_t pix = valid ? pix0 + prow + 32 * i : pix0;
            const int cc8 = chunk * 8 + oct;
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = raw[i][e];
            transform(f, cc8);
            if constexpr (YEL == OMGSR_EL_MX6) store8_mx6<T>(y, pix * 4 * C, C, cc8 * 8, f, valid);
            else if (valid) store8<T, 0>(y, pix * C + cc8 * 8, C, f);
        }
        __syncthreads();
        if (chunk + 1 < nchunk) fetch(chunk + 1);
        const u32x4_t* wc = wpk + ((int64_t)chunk * 4 * NT + wave * NTW) * 128 + lane;      // [chunk][step][column tile][hi | lo][lane]
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4_t bh[NTW], bl[NTW];
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                bh[j] = wc[(ks * NT + j) * 128];
                bl[j] = wc[(ks * NT + j) * 128 + 64];
            }
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const u32x4_t ah = thi[i * 32 * GS_ROW + arow + 2 * ks], al = tlo[i * 32 * GS_ROW + arow + 2 * ks];
                const f16x8_t ahv = *reinterpret_cast<const f16x8_t*>(&ah), alv = *reinterpret_cast<const f16x8_t*>(&al);
#pragma unroll
                for (int j = 0; j < NTW; ++j) {
                    const f16x8_t bhv = *reinterpret_cast<const f16x8_t*>(&bh[j]), blv = *reinterpret_cast<const f16x8_t*>(&bl[j]);
                    acc[i][j] = mfma32(ahv, bhv, acc[i][j]);
                    acc[i][j] = mfma32(alv, bhv, acc[i][j]);
                    acc[i][j] = mfma32(ahv, blv, acc[i][j]);
                }
            }
        }
        __syncthreads();
    }
    if (ovf && __any(amax > 65504.0f) && lane == 0) atomicOr(ovf, 1u);

    // a 32 x 32 tile at a time: fragment -> wave-private LDS tile -> rows of 16-byte stores (8 lanes cover a tile row's 128 bytes), + bias
    float* ep = reinterpret_cast<float*>(tile) + wave * (32 * GS_EP_LD);
#pragma unroll
    for (int i = 0; i < PT; ++i) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            if (i + j) __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) ep[cfrag_row(lane, r) * GS_EP_LD + (lane & 31)] = acc[i][j][r];
            __syncthreads();
            const int col = (wave * NTW + j) * 32 + (lane & 7) * 4;
            const f32x4_t b = bias ? *reinterpret_cast<const f32x4_t*>(bias + col) : (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = q * 8 + (lane >> 3);
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(ep + row * GS_EP_LD + (lane & 7) * 4);
                if (p0 + i * 32 + row < HW) *reinterpret_cast<f32x4_t*>(scout + (pix0 + i * 32 + row) * N + col) = v + b;
            }
        }
    }
}

template <int PT, int NTW>
int launch_el(const int y_el, const dim3 grid, hipStream_t st, const GnShortcutTable& m, const float* mean, const float* rstd, const float* gamma,
              const float* beta, const void* w, const float* bias, int C, int G, int act, int stat_rows, unsigned* ovf) {
    const u32x4_t* wp = (const u32x4_t*)w;
    if (y_el == OMGSR_EL_MX6) hipLaunchKernelGGL((gn_shortcut_kernel<PT, NTW, OMGSR_EL_MX6>), grid, dim3(256), 0, st, m, mean, rstd, gamma, beta, wp, bias, C, G, act, stat_rows, ovf);
    else hipLaunchKernelGGL((gn_shortcut_kernel<PT, NTW, OMGSR_EL_16>), grid, dim3(256), 0, st, m, mean, rstd, gamma, beta, wp, bias, C, G, act, stat_rows, ovf);
    return (int)hipGetLastError();
}

// pixel tile per output width: 16 PT NTW accumulator registers; 128 of them at N = 256 left the MX6 form 4 spilled registers, 96 leave none
int tile_pixels(const int N) { return N == 512 ? 64 : N == 256 ? 96 : 128; }

}  // namespace

extern "C" int32_t omgsr_groupnorm_shortcut_ok(int32_t C, int32_t N, int32_t G, int32_t y_el) {
    const bool ch = (C == 128 || C == 256 || C == 512) && (N == 128 || N == 256 || N == 512);
    return ch && G > 0 && C % G == 0 && (y_el == OMGSR_EL_16 || y_el == OMGSR_EL_MX6) && omgsr::compute_dtype() == 1;
}

extern "C" int omgsr_groupnorm_shortcut(const omgsr_gn_shortcut_group* groups, int32_t ngroups, const float* mean, const float* rstd,
                                        const float* gamma, const float* beta, const void* weight, const float* bias, int32_t C, int32_t N,
                                        int32_t G, int32_t act, int32_t stat_rows, int32_t y_el, uint32_t* overflow_flag, void* stream) {
    if (!groups || ngroups <= 0 || ngroups > OMGSR_GN_MAX_GROUPS || !mean || !rstd || !weight || C <= 0 || N <= 0 || G <= 0 || stat_rows <= 0)
        return OMGSR_E_BADARG;
    if (!omgsr_groupnorm_shortcut_ok(C, N, G, y_el) || (act != OMGSR_ACT_NONE && act != OMGSR_ACT_SILU)) return OMGSR_E_SHAPE;
    const int P = tile_pixels(N);
    GnShortcutTable m;
    memset(&m, 0, sizeof(m));
    int64_t blocks = 0;
    double pixels = 0.0;
    for (int k = 0; k < ngroups; ++k) {
        const omgsr_gn_shortcut_group& g = groups[k];
        if (!g.x || !g.y || !g.sc || g.rows <= 0 || g.HW <= 0) return OMGSR_E_BADARG;
        if (g.HW >= (1ll << 31) - P) return OMGSR_E_SHAPE;
        m.x[k] = (const float*)g.x; m.y[k] = g.y; m.sc[k] = (float*)g.sc; m.HW[k] = (int)g.HW;
        m.tiles[k] = (int)((g.HW + P - 1) / P);
        m.start[k] = (int)blocks;
        blocks += (int64_t)g.rows * m.tiles[k];
        if (blocks >= (1ll << 31)) return OMGSR_E_SHAPE;
        pixels += (double)g.rows * (double)g.HW;
    }
    m.start[ngroups] = (int)blocks;
    m.count = ngroups;
    hipStream_t st = (hipStream_t)stream;
    omgsr::TimingScope ts(OMGSR_TK_IGEMM, 2.0 * pixels * N * C, pixels * (4.0 * C + (y_el == OMGSR_EL_MX6 ? 4.0 : 2.0) * C + 4.0 * N) + 4.0 * C * N, st,
                          (long long)pixels, N, C);
    if (ts.active) ts.rec.variant = 29;
    const dim3 grid((unsigned)blocks);
    if (N == 128) return launch_el<4, 1>(y_el, grid, st, m, mean, rstd, gamma, beta, weight, bias, C, G, act, stat_rows, overflow_flag);
    if (N == 256) return launch_el<3, 2>(y_el, grid, st, m, mean, rstd, gamma, beta, weight, bias, C, G, act, stat_rows, overflow_flag);
    return launch_el<2, 4>(y_el, grid, st, m, mean, rstd, gamma, beta, weight, bias, C, G, act, stat_rows, overflow_flag);
}
