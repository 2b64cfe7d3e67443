// The thin-output 3x3 stride-1 pad-1 convolutions at the tails of the networks (conv_out: 3, 4 or 8 output channels) as an fp32 streaming
// kernel: plain fp32 FMAs on the fp32 stream tensor and the layer's unsplit fp32 weights, no MFMA, no 16-bit operand, no saturation flag.
// (Timing: kind 1, variant 28.)
//
// edge_conv_out_kernel (omgsr_conv_out_gn): GroupNorm apply + SiLU + conv with Cout <= 8 in one pass over the un-normalised map.
//   A workgroup owns an 8 x 32 tile of output pixels of one row (image or tile) and walks the input channels in chunks of 32. Per chunk the
//   (8+2) x (32+2) patch is read from HBM once (one 16-byte load per (pixel, channel quad), 128 contiguous bytes per pixel), normalised with the
//   apply kernels' algebra (a = rstd gamma, v = x a + (beta - mean a), silu_f(v): the value gn_apply_any_body rounds to 16 bits) and written to
//   LDS as [channel quad][patch pixel] float4 planes; pixels outside the map are exact zeros (the conv pads the NORMALISED map). Wave w then
//   owns channel quads 2w and 2w + 1 of the chunk for ALL 256 pixels: lane l is column l & 31 and rows 4 (l >> 5) .. + 3, reads its
//   6 x 3 window as 16-byte LDS loads (consecutive lanes, consecutive 16 bytes: conflict-free) and accumulates 4 pixels x CP outputs with
//   FMAs whose weight operand is an SGPR (the weight index is wave-uniform: scalar loads, no per-lane traffic). The next chunk's patch
//   loads are issued before the FMAs, so their latency hides under them. The four waves' partial sums meet in LDS at the end and are added in
//   wave order, then the bias: the summation order is fixed by (chunk, quad, kx, ky, channel, wave), so two launches give the same bits.
//   LDS: 8 planes x 353 float4 (odd: the 8 lanes of a pixel, one per plane, hit 8 different 4-bank groups on the way in; 352 = 11 x 32 slots,
//   so the fill needs no bounds test) = 45 184 B, three workgroups per CU.
//   Several tensors of one layer (the tiled VAE's tile-shape groups) share a launch through a prefix table of workgroup counts, the way
//   gn_apply_any_multi_kernel does it.
#include "common.hip.h"
#include "timing.hip.h"
#include "../../include/omgsr_hip.h"

namespace {

constexpr int EC_TH = 8, EC_TW = 32;                       // output tile
constexpr int EC_PW = EC_TW + 2, EC_PPIX = (EC_TH + 2) * EC_PW;      // patch: 10 x 34 = 340 pixels
constexpr int EC_PLANE = 353;                              // float4 slots per channel-quad plane: >= 32 EC_SLOTS, odd (see the header)
constexpr int EC_CK = 32;                                  // channels per chunk = 8 quads, two per wave
constexpr int EC_SLOTS = (EC_PPIX * 8 + 255) / 256;        // (pixel, quad) pairs per thread and chunk: 11 (the last one partly filled)

struct EdgeOutTable {
    const float* x[OMGSR_GN_MAX_GROUPS];
    float* y[OMGSR_GN_MAX_GROUPS];
    int H[OMGSR_GN_MAX_GROUPS], W[OMGSR_GN_MAX_GROUPS];
    int tx[OMGSR_GN_MAX_GROUPS];                           // tiles per map row
    int tiles[OMGSR_GN_MAX_GROUPS];                        // tiles per tensor row (image or tile)
    int start[OMGSR_GN_MAX_GROUPS + 1];                    // first workgroup of group k; start[count] = grid size
    int count;
};

// CP: output channels the kernel computes (4 or 8; the packed weight has that many columns - an even count, so that a v_pk_fma_f32 takes the
// weights of two neighbouring outputs as one aligned SGPR pair and broadcasts the activation: with CP = 3 the compiler spent more moves building
// register pairs than it saved FMAs). Columns CP .. 7 of the output are zeros.
template <int CP>
__global__ __launch_bounds__(256, CP == 8 ? 2 : 3) void edge_conv_out_kernel(const EdgeOutTable m, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int C, const int G, const int stat_rows) {
    __shared__ __attribute__((aligned(16))) f32x4_t patch[8 * EC_PLANE];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int s = 0;
    while (s + 1 < m.count && (int)blockIdx.x >= m.start[s + 1]) ++s;          // wave-uniform
    const int local = (int)blockIdx.x - m.start[s];
    const int n = local / m.tiles[s], tile = local - n * m.tiles[s];
    const int H = m.H[s], W = m.W[s];
    const int y0 = (tile / m.tx[s]) * EC_TH, x0 = (tile % m.tx[s]) * EC_TW;
    const float* __restrict__ xb = m.x[s] + (int64_t)n * H * W * C;
    const int ns = n % stat_rows;              // tiled VAE: rows are (tile, image) tile-major and share the image's statistics
    const int cpg = C / G;

    // this thread's patch slots: quad q of patch pixels (t >> 3) + 32 i. Branch-free: a slot outside the map (or past the patch: the planes
    // have room for 32 EC_SLOTS pixels) loads the map's first pixel instead and is zeroed on the way into LDS (bit i of `inside` clear)
    const int q = t & 7;
    int off[EC_SLOTS];
    unsigned inside = 0;
#pragma unroll
    for (int i = 0; i < EC_SLOTS; ++i) {
        const int p = (t >> 3) + 32 * i;
        const int gy = y0 - 1 + p / EC_PW, gx = x0 - 1 + p % EC_PW;
        const bool in = p < EC_PPIX && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        off[i] = in ? (gy * W + gx) * C : 0;
        inside |= in ? 1u << i : 0u;
    }
    f32x4_t raw[EC_SLOTS];
    auto fetch = [&](const int chunk) {
#pragma unroll
        for (int i = 0; i < EC_SLOTS; ++i) raw[i] = *reinterpret_cast<const f32x4_t*>(xb + off[i] + chunk * EC_CK + q * 4);
    };

    float acc[4][CP];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int co = 0; co < CP; ++co) acc[o][co] = 0.0f;
    const int win0 = (4 * (lane >> 5)) * EC_PW + (lane & 31);      // patch pixel of the window's top-left corner

    const int nchunk = C / EC_CK;
    fetch(0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        // (scale, shift) of this thread's four channels: the two expressions of the apply kernels
        float sc[4], sh[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = chunk * EC_CK + q * 4 + e, g = c / cpg;
            const float r = rstd[ns * G + g], mu = mean[ns * G + g];
            const float a = r * gamma[c];
            sc[e] = a;
            sh[e] = beta[c] - mu * a;
        }
#pragma unroll
        for (int i = 0; i < EC_SLOTS; ++i) {
            f32x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = silu_f((inside >> i & 1u) ? raw[i][e] * sc[e] + sh[e] : 0.0f);      // silu_f(0) = +0
            patch[q * EC_PLANE + (t >> 3) + 32 * i] = v;
        }
        __syncthreads();
        if (chunk + 1 < nchunk) fetch(chunk + 1);
#pragma unroll 1
        for (int j = 0; j < 2; ++j) {
            const int cq = wave * 2 + j;
            const float* __restrict__ wq = w + (int64_t)((chunk * 8 + cq) * 9) * 4 * CP;      // [ky][kx][channel of the quad][CP], wave-uniform
            const f32x4_t* pl = patch + cq * EC_PLANE + win0;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                f32x4_t a[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) a[r] = pl[r * EC_PW + kx];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int co = 0; co < CP; ++co) {
                            const float wv = wq[((ky * 3 + kx) * 4 + e) * CP + co];
#pragma unroll
                            for (int o = 0; o < 4; ++o) acc[o][co] = fmaf(a[o + ky][e], wv, acc[o][co]);
                        }
            }
        }
        __syncthreads();
    }

    // the four waves' partial sums, added in wave order; wave w then stores row w of every lane's four
    float* red = reinterpret_cast<float*>(patch);              // [wave][row][co][lane]: 4 x 4 x CP x 64 floats <= 32 KB
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int co = 0; co < CP; ++co) red[((wave * 4 + o) * CP + co) * 64 + lane] = acc[o][co];
    __syncthreads();
    const int gy = y0 + 4 * (lane >> 5) + wave, gx = x0 + (lane & 31);
    float out[8];
#pragma unroll
    for (int co = 0; co < 8; ++co) {
        out[co] = 0.0f;
        if (co < CP) {
            const float* r = red + (wave * CP + co) * 64 + lane;
            out[co] = ((r[0] + r[4 * CP * 64]) + (r[8 * CP * 64] + r[12 * CP * 64])) + (bias ? bias[co] : 0.0f);
        }
    }
    if (gy < H && gx < W) {
        float* o = m.y[s] + (((int64_t)n * H + gy) * W + gx) * 8;
        *reinterpret_cast<f32x4_t*>(o) = (f32x4_t){out[0], out[1], out[2], out[3]};
        *reinterpret_cast<f32x4_t*>(o + 4) = (f32x4_t){out[4], out[5], out[6], out[7]};
    }
}


}  // namespace

extern "C" int omgsr_conv_out_gn(const omgsr_edge_group* groups, int32_t ngroups, const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, const float* weight, const float* bias, int32_t Cin, int32_t Cout, int32_t G,
                                 int32_t stat_rows, void* stream) {
    if (!groups || ngroups <= 0 || ngroups > OMGSR_GN_MAX_GROUPS || !mean || !rstd || !gamma || !beta || !weight || Cin <= 0 || Cout <= 0 || G <= 0 || stat_rows <= 0)
        return OMGSR_E_BADARG;
    if ((Cin % EC_CK) || Cin > 1024 || (Cin % G) || Cout > 8) return OMGSR_E_SHAPE;
    EdgeOutTable m;
    memset(&m, 0, sizeof(m));
    int64_t blocks = 0;
    double pixels = 0.0;
    for (int k = 0; k < ngroups; ++k) {
        const omgsr_edge_group& g = groups[k];
        if (!g.x || !g.y || g.rows <= 0 || g.H <= 0 || g.W <= 0) return OMGSR_E_BADARG;
        if ((int64_t)g.H * g.W * Cin >= (1ll << 31)) return OMGSR_E_SHAPE;          // 32-bit element offsets inside a row
        m.x[k] = (const float*)g.x; m.y[k] = (float*)g.y; m.H[k] = g.H; m.W[k] = g.W;
        m.tx[k] = (g.W + EC_TW - 1) / EC_TW;
        m.tiles[k] = m.tx[k] * ((g.H + EC_TH - 1) / EC_TH);
        m.start[k] = (int)blocks;
        blocks += (int64_t)g.rows * m.tiles[k];
        if (blocks >= (1ll << 31)) return OMGSR_E_SHAPE;
        pixels += (double)g.rows * g.H * g.W;
    }
    m.start[ngroups] = (int)blocks;
    m.count = ngroups;
    hipStream_t st = (hipStream_t)stream;
    omgsr::TimingScope ts(OMGSR_TK_IGEMM, 2.0 * pixels * Cout * 9.0 * Cin, pixels * (4.0 * Cin + 32.0) + 36.0 * Cin * Cout, st,
                          (long long)pixels, 8, 9ll * Cin);
    if (ts.active) ts.rec.variant = 28;
    const dim3 grid((unsigned)blocks), block(256);
    if (Cout <= 4) hipLaunchKernelGGL(edge_conv_out_kernel<4>, grid, block, 0, st, m, mean, rstd, gamma, beta, weight, bias, Cin, G, stat_rows);
    else hipLaunchKernelGGL(edge_conv_out_kernel<8>, grid, block, 0, st, m, mean, rstd, gamma, beta, weight, bias, Cin, G, stat_rows);
    return (int)hipGetLastError();
}
