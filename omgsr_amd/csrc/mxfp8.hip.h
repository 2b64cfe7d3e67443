// The OMGSR_EL_MXFP8 element rule (include/omgsr_hip.h), shared by the quantiser (gemm_mxfp8.hip) and the kernels that write the form
// directly (norm.hip: rmsnorm_rope_mxfp8_kernel, gn_apply_mxfp8_kernel, the LayerNorm's LnMx8 forms; igemm_epilogue.hip.h: OUT8).
#pragma once
#include "common.hip.h"

// fp32 -> OCP e4m3fn, round to nearest even, |a| <= 448 (the caller clamps): the conversion of c10::Float8_e4m3fn, bit for bit
OMGSR_DEVINL unsigned e4m3_rne(const float v) {
    const unsigned bits = __float_as_uint(v);
    const unsigned sign = (bits >> 24) & 0x80u;
    const float a = __uint_as_float(bits & 0x7fffffffu);
    unsigned code;
    if (a < 0.015625f) {                                // below 2^-6: subnormal codes m 2^-9 (m = 8 is the smallest normal, code 8)
        code = (unsigned)__builtin_rintf(a * 512.0f);
    } else {
        unsigned b = __float_as_uint(a);
        b += 0x7ffffu + ((b >> 20) & 1u);               // round the 23-bit mantissa to 3 bits, ties to even
        code = (b >> 20) - ((127u - 7u) << 3);
    }
    return sign | code;
}

// E8M0 scale of a block whose largest magnitude is mx: max(0, biased exponent - 8)
OMGSR_DEVINL int mxfp8_scale(const float mx) {
    const int e = (int)((__float_as_uint(mx) >> 23) & 0xffu);
    return e > 8 ? e - 8 : 0;
}

// code of v under scale s: (v 2^(127 - s)).clamp(-448, 448) in e4m3fn
OMGSR_DEVINL unsigned mxfp8_code(const float v, const int s) {
    const float mul = __uint_as_float((unsigned)(254 - s) << 23);      // 2^(127 - s): a normal float for every s in [0, 246]
    return e4m3_rne(fminf(fmaxf(v * mul, -448.0f), 448.0f));
}

// A fused producer's octet: the lane's 8 fp32 results rounded to bf16 by the 16-bit store's own conversion (pack8<bf16_t>), then the quantiser's
// rule on those rounded values - the bytes of "store bf16, run omgsr_quantize_mxfp8". The four octets of the 32-value block sit in one lane quad
// (consecutive lanes = consecutive octets, the quad all-live): its maximum is two exchanges. Returns the codes; s = the block's E8M0 byte.
OMGSR_DEVINL u32x2_t mxfp8_quad_octet(const float (&v)[8], int& s) {
    float f[8];
    unpack8<bf16_t>(pack8<bf16_t>(v), f);
    float mx = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(f[e]));
    s = mxfp8_scale(quad_max(mx));
    u32x2_t out = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e >> 2] |= mxfp8_code(f[e], s) << (8 * (e & 3));
    return out;
}
