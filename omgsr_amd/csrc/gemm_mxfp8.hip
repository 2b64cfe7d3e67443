// MXFP8 x MXFP8 token GEMM (the fp8 tier's DiT linears) and the MXFP8 quantiser (include/omgsr_hip.h, OMGSR_EL_MXFP8).
//
// mxfp8_gemm_kernel runs igemm_p8_kernel's schedule on fp8 codes: 256 x 256 tile, 8 waves in two groups half a phase apart, LDS-DMA
// half-tiles with the XOR-swizzled 16-byte slots (see igemm_p8.hip for the schedule itself). What changes:
//  * a 128-byte LDS row holds 128 fp8 values of K (p8: 64 bf16), so BK = 128 and a K-tile is half as many tiles for the same K;
//  * each phase runs 2 x 2 v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, 16 passes) where p8 runs 8 bf16 32x32x16 MFMAs: the same
//    matrix-pipe time per phase, twice the K. Operand map of the instruction (e4m3, measured with one-hot codes and per-lane scales):
//    lane l (row l & 31, half h = l >> 5) holds K 16 h .. 16 h + 15 of the 64 in its registers 0-3 and K 32 + 16 h .. + 15 in registers 4-7,
//    and the scale of K block b (0, 1) is taken from lane half b. So k-step s reads chunks 4 s + h and 4 s + 2 + h of a row (hardware
//    blocks 0 / 1 = the format's blocks 2 s / 2 s + 1) and lane half h supplies the E8M0 byte of block 2 s + h;
//  * the scales of a K-tile (4 bytes per row, one dword) travel with it: one extra dword LDS-DMA piece per wave per K-tile (waves 0-3
//    the 256 operand rows, waves 4-7 the 256 weight rows) issued in the phase that stages the tile's second A half-tile, so the counted
//    vmcnt(4) waits of the schedule still cover it. A lane reads the dwords of its rows and shifts its block's byte down (v_bfe).
// Odd K-tile counts run the last pair's second half as barriers and DMA pieces without MFMAs. The epilogue is igemm_epilogue_linear.
#include "gemm_mxfp8_body.hip.h"

namespace {

__global__ __launch_bounds__(512, 2) void mxfp8_gemm_kernel(const omgsr_igemm_args p, const IgemmGeo g) {
    mxfp8_gemm_body<false>(p, g, xcd_remap(blockIdx.x, g.ntm * g.ntn), blockIdx.z);
}

// ---- quantiser: one thread per 32-element block ----------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void mxfp8_quantize_kernel(const TI* __restrict__ x, const int64_t rows, const int K, const int64_t x_ld,
                                                             unsigned char* __restrict__ codes, unsigned char* __restrict__ scales,
                                                             const int64_t c_ld, const int64_t s_ld) {
    const int nb = K >> 5;
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= rows * nb) return;
    const int64_t r = id / nb;
    const int b = (int)(id - r * nb);
    const TI* src = x + r * x_ld + 32 * b;
    float v[32];
    if constexpr (std::is_same<TI, float>::value) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 q = reinterpret_cast<const float4*>(src)[i];
            v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 q = reinterpret_cast<const uint4*>(src)[i];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[8 * i + 2 * k] = __uint_as_float(w[k] << 16);
                v[8 * i + 2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
            }
        }
    }
    float mx = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) mx = fmaxf(mx, fabsf(v[i]));
    const int s = mxfp8_scale(mx);
    unsigned out[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= mxfp8_code(v[4 * i + k], s) << (8 * k);
        out[i] = w;
    }
    uint4* dst = reinterpret_cast<uint4*>(codes + r * c_ld + 32 * b);
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
    scales[r * s_ld + b] = (unsigned char)s;
}

}  // namespace

namespace omgsr {
// What mxfp8_gemm_kernel runs (omgsr_igemm refuses every other mxf8 problem with OMGSR_E_SHAPE)
bool mxfp8_gemm_ok(const omgsr_igemm_args& a) {
    const int64_t M = (int64_t)a.N * a.Ho * a.Wo;
    return a.R == 1 && a.S == 1 && a.stride == 1 && a.pad_top == 0 && a.pad_left == 0 && a.upsample == 0 && a.Ho == a.H && a.Wo == a.W &&
           a.K_pad == a.Cin && (a.Cin % BK) == 0 && (a.in_ld == 0 || a.in_ld == a.Cin) && (a.Cout_pad % BN) == 0 && a.act != OMGSR_ACT_GEGLU &&
           !a.in_split && !a.w_split && a.mx_chunks16 == 0 && a.out_mx == 0 && !a.gn_partial && !a.gn_scale_shift && !a.weight_cm && !a.weight_ph &&
           a.in_scale && a.w_scale && compute_dtype() == 0 && (a.in_bstride % 32) == 0 && (a.w_bstride % 32) == 0 &&
           M * a.Cin < (1ll << 32) && (int64_t)a.Cout_pad * a.K_pad < (1ll << 32);
}

int mxfp8_gemm_launch(const omgsr_igemm_args& a, IgemmGeo g, hipStream_t st) {
    g.ntm = (g.M + BM - 1) / BM;
    g.ntn = (a.Cout + BN - 1) / BN;
    g.splits = 1;
    return launch_lds<mxfp8_gemm_kernel>(dim3(g.ntm * g.ntn, 1, a.batch), dim3(512), LDS_BYTES, st, a, g);
}
}  // namespace omgsr

namespace {
int quantize_launch(const void* x, int32_t x_el, int64_t rows, int32_t K, int64_t x_ld, void* codes, void* scales, int64_t c_ld, int64_t s_ld, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    omgsr::TimingScope ts(OMGSR_TK_ELT, 0.0, (double)rows * K * ((x_el == OMGSR_EL_F32 ? 4.0 : 2.0) + 1.0 + 1.0 / 32.0), st);
    const int64_t n = rows * (K / 32);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (x_el == OMGSR_EL_F32)
        hipLaunchKernelGGL((mxfp8_quantize_kernel<float>), grid, dim3(256), 0, st, (const float*)x, rows, (int)K, x_ld, (unsigned char*)codes, (unsigned char*)scales,
                           c_ld, s_ld);
    else
        hipLaunchKernelGGL((mxfp8_quantize_kernel<unsigned short>), grid, dim3(256), 0, st, (const unsigned short*)x, rows, (int)K, x_ld, (unsigned char*)codes,
                           (unsigned char*)scales, c_ld, s_ld);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int omgsr_quantize_mxfp8(const void* x, int32_t x_el, int64_t rows, int32_t K, int64_t x_ld, void* codes, void* scales, void* stream) {
    if (!x || !codes || !scales || rows <= 0 || K <= 0 || (x_el != OMGSR_EL_16 && x_el != OMGSR_EL_F32)) return OMGSR_E_BADARG;
    if ((K % 128) || x_ld < K || (x_ld & 7)) return OMGSR_E_SHAPE;
    return quantize_launch(x, x_el, rows, K, x_ld, codes, scales, K, K / 32, stream);
}

extern "C" int omgsr_quantize_mxfp8_ld(const void* x, int32_t x_el, int64_t rows, int32_t K, int64_t x_ld, void* codes, void* scales, int64_t c_ld,
                                       int64_t s_ld, void* stream) {
    if (!x || !codes || !scales || rows <= 0 || K <= 0 || (x_el != OMGSR_EL_16 && x_el != OMGSR_EL_F32)) return OMGSR_E_BADARG;
    if ((K % 128) || x_ld < K || (x_ld & 7) || c_ld < K || (c_ld & 15) || s_ld < K / 32 || ((uintptr_t)codes & 15)) return OMGSR_E_SHAPE;
    return quantize_launch(x, x_el, rows, K, x_ld, codes, scales, c_ld, s_ld, stream);
}
