// ESM-2 masked-LM head (opus_esm2_lm_head): logits = LN(gelu_erf(h Wd^T + bd)) We^T + b over enc_vocab (33) columns.
//   mlm_gather_kernel : the selected fp32 rows of the encoder's final states -> operand rows of the dense GEMM (which runs
//                       through the GEMM router with the erf-GELU epilogue, as the encoder's fc1 does)
//   mlm_head_kernel   : LayerNorm (fp32, two-pass), the 33 dot products of length De (fp32 accumulation), the bias and
//                       optionally the log-softmax over the columns, ONE launch, fp32 [R, V] out
// The 33 columns run on vector FMAs, one wave per row: the row stays in registers from the LayerNorm on, the table We
// (V x De operands: 84 KB at De = 1280, 165 KB at 2560 - more than a CU's LDS) is read through L1 / L2, 8-byte loads that
// the four waves of a workgroup issue almost together.  An MFMA form would pad N to 48, need the normalised row rounded to
// the 16-bit operand type, and save nothing that shows: the head is 2 V De flops per row, under 3 % of the dense step.
#include "common.h"

namespace opus {

__device__ __forceinline__ float mlm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float mlm_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per output row m < Mg.  m < R: row idx[m] (idx null: row m) of src, cast to the operand type; an index outside
// [0, src_rows) gives a NaN row (the logits of that row are then NaN: no silent read of another row).  R <= m < Mg: zeros (the
// padding rows of a fixed-shape GEMM launch).
__global__ __launch_bounds__(256) void mlm_gather_kernel(const float *__restrict__ src, int64_t src_rows, const int32_t *__restrict__ idx,
                                                         int R, int Mg, int D, half_t *__restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int nvec = D >> 2;
    for (int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); m < Mg; m += (int64_t)gridDim.x * 4) {
        h4 *out = reinterpret_cast<h4 *>(dst + m * D);
        int64_t r = -1;
        float fill = 0.f;
        if (m < R) {
            r = idx ? (int64_t)idx[m] : m;
            if (r < 0 || r >= src_rows) { r = -1; fill = __builtin_nanf(""); }
        }
        if (r < 0) {
            const h4 z = {(half_t)fill, (half_t)fill, (half_t)fill, (half_t)fill};
            for (int c = lane; c < nvec; c += 64) out[c] = z;
            continue;
        }
        const float4 *in = reinterpret_cast<const float4 *>(src + r * D);
        for (int c = lane; c < nvec; c += 64) {
            const float4 v = in[c];
            const h4 o = {(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
            out[c] = o;
        }
    }
}

hipError_t launch_mlm_gather(const float *src, int64_t src_rows, const int32_t *idx, int R, int Mg, int D, half_t *dst, hipStream_t s) {
    if (R < 0 || Mg < 1 || R > Mg || D < 4 || (D & 3)) return hipErrorInvalidValue;
    const int blocks = (int)(cdiv((int64_t)Mg, 4) < 2048 ? cdiv((int64_t)Mg, 4) : 2048);
    OPUS_LAUNCH(KC_MLM, mlm_gather_kernel, dim3(blocks), dim3(256), 0, s, src, src_rows, idx, R, Mg, D, dst);
    return hipGetLastError();
}

// NV = 4-element groups per lane (rows up to 256 NV columns), as norm.hip's row kernels: the row lives in exactly the registers
// it needs.  One wave per row, rows strided over the grid; lane n < V ends up holding logit n.
template <int NV>
__global__ __launch_bounds__(256) void mlm_head_kernel(const half_t *__restrict__ y, const float *__restrict__ lnw,
                                                       const float *__restrict__ lnb, float eps, const half_t *__restrict__ We,
                                                       const float *__restrict__ bias, int64_t R, int D, int V, int log_softmax,
                                                       float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int nvec = D >> 2;
    const float4 *wr = reinterpret_cast<const float4 *>(lnw);
    const float4 *br = reinterpret_cast<const float4 *>(lnb);
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (int64_t)gridDim.x * 4) {
        const h4 *yr = reinterpret_cast<const h4 *>(y + row * D);
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 64 + lane;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < nvec) {
                const h4 t = yr[c];
                v[i] = make_float4((float)t.x, (float)t.y, (float)t.z, (float)t.w);
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            }
        }
        const float mean = mlm_wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 64 + lane;
            if (c < nvec) {
                const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
                q += (a * a + b * b) + (cc * cc + d * d);
            }
        }
        const float rstd = rsqrtf(mlm_wave_sum(q) / D + eps);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 64 + lane;
            if (c < nvec) {
                const float4 g = wr[c], b = br[c];
                v[i].x = (v[i].x - mean) * rstd * g.x + b.x; v[i].y = (v[i].y - mean) * rstd * g.y + b.y;
                v[i].z = (v[i].z - mean) * rstd * g.z + b.z; v[i].w = (v[i].w - mean) * rstd * g.w + b.w;
            }
        }
        float mine = -INFINITY;
        for (int n = 0; n < V; ++n) {
            const h4 *er = reinterpret_cast<const h4 *>(We + (int64_t)n * D);
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = i * 64 + lane;
                if (c < nvec) {
                    const h4 w = er[c];
                    a0 = __builtin_fmaf(v[i].x, (float)w.x, a0); a1 = __builtin_fmaf(v[i].y, (float)w.y, a1);
                    a0 = __builtin_fmaf(v[i].z, (float)w.z, a0); a1 = __builtin_fmaf(v[i].w, (float)w.w, a1);
                }
            }
            const float t = mlm_wave_sum(a0 + a1);
            if (lane == n) mine = t + bias[n];
        }
        if (log_softmax) {
            const float mx = mlm_wave_max(mine);                       // (lanes >= V hold -inf: exp -> 0)
            const float z = mlm_wave_sum(lane < V ? expf(mine - mx) : 0.f);
            mine = (mine - mx) - logf(z);
        }
        if (lane < V) out[row * V + lane] = mine;
    }
}

hipError_t launch_mlm_head(const half_t *y, const float *lnw, const float *lnb, float eps, const half_t *We, const float *bias,
                           int64_t R, int D, int V, int log_softmax, float *out, hipStream_t s) {
    if (R < 1 || D < 4 || (D & 3) || D > 20 * 256 || V < 1 || V > 64) return hipErrorInvalidValue;
    // few rows: one workgroup per four rows (a single workgroup up to R = 4); many rows: eight workgroups per CU walk them
    const int64_t want = cdiv(R, 4);
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
#define OPUS_MLM_GO(NV) OPUS_LAUNCH(KC_MLM, (mlm_head_kernel<NV>), grid, block, 0, s, y, lnw, lnb, eps, We, bias, R, D, V, log_softmax, out)
    if (D <= 256) OPUS_MLM_GO(1);
    else if (D <= 5 * 256) OPUS_MLM_GO(5);
    else if (D <= 10 * 256) OPUS_MLM_GO(10);
    else OPUS_MLM_GO(20);
#undef OPUS_MLM_GO
    return hipGetLastError();
}

}  // namespace opus
