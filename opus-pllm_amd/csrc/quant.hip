// Load-time FP8 quantiser of the decoder-layer weights ("FP8 panels"; tests/w8_ref.py is the CPU twin).
//
// W[N][K] in the operand type, row-major, after all load-time fusion ->
//   e8[n]     int8: the smallest e with absmax_n 2^-e <= 448 (= 1.75 2^8: the largest e4m3fn value), read off the exponent and
//             mantissa fields of absmax_n; 0 for an all-zero row; never below W8_EXP_MIN (reachable by bf16 rows of |w| < 2^-112 only)
//   q8        OCP e4m3fn codes q = RNE(W 2^-e) in the FP8 panel layout (fp8_tiled_off); the scaling is exact, |W 2^-e| <= 448, so
//             no code saturates and none is NaN (0x7f / 0xff); a code whose value q 2^e would be subnormal in the operand type is +0
//   dq        q 2^e in the operand type, row-major (exact: 4 significant bits, normal by the rule above)
//             (and a code that RNE carried past the operand type's largest finite value - fp16 weights of |w| >= 63488 - is the
//             next code towards zero, so that dq stays finite)
// A non-finite weight sets *bad and every code of the call is +0.
#include "common.h"

namespace opus {

// biased exponent and mantissa fields of a positive normal fp32 -> smallest e with a 2^-e <= 448
__device__ __forceinline__ int row_exponent(float absmax) {
    const uint32_t b = __builtin_bit_cast(uint32_t, absmax);
    if (b < 0x00800000u) return 0;                            // zero (or an fp32 subnormal: bf16 rows whose codes are all +0 anyway)
    const int e = (int)(b >> 23) - 127 - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);     // mantissa above 1.75: one more
    return e < W8_EXP_MIN ? W8_EXP_MIN : e;
}

// one wave per row: absmax -> e8
__global__ __launch_bounds__(256) void fp8_row_exponent_kernel(const half_t *__restrict__ src, int64_t N, int64_t K,
                                                               int8_t *__restrict__ e8, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float mx = 0.f;
    bool nonfinite = false;
    for (int64_t k = lane * 8; k < K; k += 512) {
        const h8 v = *reinterpret_cast<const h8 *>(src + n * K + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = fabsf((float)v[j]);
            nonfinite |= !(a <= 3.4e38f);                    // inf or NaN
            mx = fmaxf(mx, a);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (__any(nonfinite)) {
        if (lane == 0) { *bad = 1; e8[n] = 0; }
        return;
    }
    if (lane == 0) e8[n] = (int8_t)row_exponent(mx);
}

// RNE of |v| <= 448 to an e4m3fn code (sign in bit 7).  Below the smallest normal 2^-6 the codes step by 2^-9.
__device__ __forceinline__ uint32_t e4m3_rne(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    const uint32_t sign = (b >> 24) & 0x80u, mag = b & 0x7fffffffu;
    uint32_t code;
    if (mag < 0x3c800000u) {                                  // |v| < 2^-6
        code = (uint32_t)(int)rintf(__builtin_bit_cast(float, mag) * 512.0f);       // 0 .. 8 (8 = the smallest normal)
    } else {
        const uint32_t r = mag + 0x7ffffu + ((mag >> 20) & 1u);                      // ties to the even 3-bit mantissa
        code = (r >> 20) - ((127u - 7u) << 3);
    }
    return sign | code;
}

// value of a non-NaN e4m3fn magnitude code (0 .. 0x7e) as fp32, and its binary exponent floor(log2)
__device__ __forceinline__ float e4m3_value(uint32_t code, int &xq) {
    const int ex = (int)(code >> 3), m = (int)(code & 7);
    if (ex == 0) {
        xq = m ? 31 - __builtin_clz(m) - 9 : -1000;
        return (float)m * (1.0f / 512.0f);
    }
    xq = ex - 7;
    return __builtin_bit_cast(float, (uint32_t)((ex - 7 + 127) << 23) | ((uint32_t)m << 20));
}

// one thread per 8 consecutive k of a row: 16 B of W in, 8 B of codes (their place in the panel) and 16 B of dq out
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const half_t *src, int64_t N, int64_t K,   // (dq may be src: no restrict)
                                                           const int8_t *__restrict__ e8, const int *__restrict__ bad,
                                                           uint8_t *__restrict__ q8, half_t *dq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * (K >> 3)) return;
    const int64_t n = i / (K >> 3), k = (i % (K >> 3)) * 8;
    const int e = e8[n];
    const bool zero_all = *bad != 0;                          // (the caller reports the error; nothing of this call is to be used)
    const h8 w = *reinterpret_cast<const h8 *>(src + n * K + k);
    h8 d;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t code = zero_all ? 0u : e4m3_rne(ldexpf((float)w[j], -e));
        int xq;
        float v = e4m3_value(code & 0x7fu, xq);
        if (xq + e > OPERAND_MAX_EXP) v = e4m3_value((--code) & 0x7fu, xq);   // rounded up past the largest finite operand: one code back
        if (xq + e < OPERAND_MIN_EXP) { code = 0; v = 0.f; }  // would be subnormal (or is zero) in the operand type: +0
        v = ldexpf(code & 0x80u ? -v : v, e);
        d[j] = (half_t)v;
        if (j < 4) lo |= code << (8 * j); else hi |= code << (8 * (j - 4));
    }
    *reinterpret_cast<uint2 *>(q8 + fp8_tiled_off(n, k, K)) = make_uint2(lo, hi);
    if (dq) *reinterpret_cast<h8 *>(dq + n * K + k) = d;
}

hipError_t launch_quantize_fp8(const half_t *src, int64_t N, int64_t K, uint8_t *q8, int8_t *e8, half_t *dq, int *bad, hipStream_t s) {
    hipLaunchKernelGGL(fp8_row_exponent_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, src, N, K, e8, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fp8_quantize_kernel, dim3(cdiv(N * (K >> 3), 256)), dim3(256), 0, s, src, N, K, e8, bad, q8, dq);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ MXFP4
// Load-time MXFP4 quantiser ("MXFP4 panels"; tests/w4_ref.py is the CPU twin).  A block is 32 consecutive k of
// one row:
//   s4   the e8m0 scale byte e + 127, e = floor(log2(absmax_block)) - 2 read off the fp32 exponent field of absmax_block (the OCP
//        MX v1.0 rule: the largest e2m1 value is 1.5 2^2); never below W4_EXP_MIN; 0 for an all-zero block (and for an absmax below
//        the smallest normal fp32: bf16 only)
//   q4   e2m1 codes, magnitude RNE(min(|w| 2^-e, 6)) over {0, 0.5, 1, 1.5, 2, 3, 4, 6} with ties to the even code, sign in bit 3,
//        two per byte (the lower k in the low nibble), in the code panels (mx4_code_off); a code whose value q 2^e would be
//        subnormal in the operand type is +0, and so is a negative zero
//   dq   q 2^e in the operand type, row-major (exact: 2 significant bits, normal by the rule above, at most 1.5 2^(e + 2) <= absmax)
// All of it in integer arithmetic on the fp32 bits of the weights.  A non-finite weight sets *bad; its block's codes are +0.
//
// One thread per 8 consecutive k of a row (16 B of W in, 4 B of codes and 16 B of dq out); the four threads of a block are four
// neighbouring lanes of one wave (K % 64 == 0, so N K / 8 is a multiple of 128: whole waves leave at the bounds check).
__global__ __launch_bounds__(256) void mxfp4_quantize_kernel(const half_t *src, int64_t N, int64_t K,   // (dq may be src: no restrict)
                                                             uint8_t *__restrict__ q4, uint8_t *__restrict__ s4, half_t *dq,
                                                             int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * (K >> 3)) return;
    const int64_t n = i / (K >> 3), k = (i % (K >> 3)) * 8;
    const h8 w = *reinterpret_cast<const h8 *>(src + n * K + k);
    uint32_t mag[8], mx = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mag[j] = __builtin_bit_cast(uint32_t, (float)w[j]) & 0x7fffffffu;
        mx = mag[j] > mx ? mag[j] : mx;                       // (non-negative floats order as their bits)
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {                        // the block's four lanes
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    const bool nonfinite = mx >= 0x7f800000u;                 // inf or NaN somewhere in the block
    int e = 0;
    if (mx >= 0x00800000u) {
        e = (int)(mx >> 23) - 127 - 2;
        e = e < W4_EXP_MIN ? W4_EXP_MIN : e;
    }
    if (nonfinite) { *bad = 1; e = 0; }
    h8 d;
    uint32_t codes = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // v = |w| 2^-e as fp32 bits (exact: the exponent field moves); below the smallest normal fp32 it rounds to 0 anyway
        const int ex = (int)(mag[j] >> 23);
        uint32_t m = 0;
        if (!nonfinite && ex > 0 && ex - e > 0) {
            const uint32_t v = mag[j] - ((uint32_t)e << 23);
            // nearest of the 8 magnitudes, ties to the even code: (0.25, 0.75) -> 0.5, [0.75, 1.25] -> 1, (1.25, 1.75) -> 1.5,
            // [1.75, 2.5] -> 2, (2.5, 3.5) -> 3, [3.5, 5] -> 4, above 5 -> 6 (saturating)
            m = (v > 0x3e800000u) + (v >= 0x3f400000u) + (v > 0x3fa00000u) + (v >= 0x3fe00000u) + (v > 0x40200000u) +
                (v >= 0x40600000u) + (v > 0x40a00000u);
        }
        const int xq = m == 1 ? -1 : (int)(m >> 1) - 1;      // binary exponent of the magnitude (m > 0)
        if (m == 0 || xq + e < OPERAND_MIN_EXP) m = 0;        // zero, or subnormal in the operand type: +0
        uint32_t vb = 0, code = 0;
        if (m) {
            const uint32_t sign = __builtin_bit_cast(uint32_t, (float)w[j]) >> 31;
            code = m | (sign << 3);
            vb = (sign << 31) | ((uint32_t)(xq + e + 127) << 23) | ((m >= 2 && (m & 1)) ? 0x400000u : 0u);
        }
        d[j] = (half_t)__builtin_bit_cast(float, vb);
        codes |= code << (4 * j);
    }
    *reinterpret_cast<uint32_t *>(q4 + mx4_code_off(n, k, K)) = codes;
    if ((k & 31) == 0) s4[mx4_scale_off(n, k >> 5, K)] = (uint8_t)(e + 127);
    if (dq) *reinterpret_cast<h8 *>(dq + n * K + k) = d;
}

hipError_t launch_quantize_mxfp4(const half_t *src, int64_t N, int64_t K, uint8_t *q4, uint8_t *s4, half_t *dq, int *bad, hipStream_t s) {
    hipLaunchKernelGGL(mxfp4_quantize_kernel, dim3(cdiv(N * (K >> 3), 256)), dim3(256), 0, s, src, N, K, q4, s4, dq, bad);
    return hipGetLastError();
}

}  // namespace opus
