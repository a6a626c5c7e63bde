// Classifier-free guidance on paired rows (generate(guidance_scale=g), transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor):
// a guided call of P prompts runs 2 P decoder rows, rows [0, P) the conditional prompts and rows [P, 2 P) the negative prompts.
// At the head of every step, before the other logits processors, row b becomes
//     s = g ((l_c - lse_c) - (l_u - lse_u)) + (l_u - lse_u)
// in fp32 (HF's expression on the two log-softmaxes), l_u being row P + b, which is left as it is.  A log-softmax is taken as
// (l - max) - log(sum exp(l - max)), the row's maximum and the logarithm kept apart: l - lse with one rounded lse loses half an ulp
// of the lse (5e-4 for logits around 1e4), the shifted form is as exact as torch's.  The selection, the processors,
// the constraint and the sampling head then run on the P head rows, and row P + b is fed the token chosen for row b.
//
//   guidance_lse_partial_kernel grid (APART parts, rows): the part's maximum and sum of exp(l - part max), one pass, every thread
//                             adding its ids in an order that depends on the ids alone, never on the row's address: two
//                             bit-equal rows get bit-equal sums wherever they lie, so that a pair of equal rows gives
//                             g 0 + u = u exactly (argmax_lse_partial_kernel gives aligned rows and the others two different
//                             summation orders).  16-byte loads where the part is aligned (every row when V % 4 == 0, the
//                             decode step's case), single loads of the same ids elsewhere.
//   guidance_lse_final_kernel one wave per row: the row's maximum, log(sum exp(l - max)) and their sum (the log-sum-exp the step
//                             kernel subtracts from the chosen id's raw logit) from the APART parts, in a fixed order.
//   guidance_combine_kernel   grid (pairs, slices): several workgroups per row - 32 rows of 128 256 ids from 32 CUs would take
//                             the time of an eighth of the chip (constraint.hip measured that for its one-workgroup-per-row
//                             form).  About 12 bytes per id and pair (16 with `keep`).  Rows need no alignment (V odd): the
//                             slice is cut into up to 3 single ids, groups of four at 16-byte aligned addresses of the
//                             conditional row, and a tail; the partner row (and `keep`) take 16-byte accesses when their
//                             address has the same phase and single elements otherwise.  g is read from a device word: a new
//                             value needs no new captured step.
//                             keep != nullptr: the raw conditional row is copied there first (output_token_logprobs stays raw
//                             and conditional; the step kernel reads the chosen id's raw logit from it).
//   guidance_pair_next_kernel next[P + b] = next[b]: the partner decodes the token chosen for row b, pads after it finished included.
#include "common.h"

namespace opus {

constexpr int GD_THREADS = 256;

// (one fused multiply-add, spelled out: g * 0 + u == u exactly for a pair of bit-equal rows, whatever the compiler contracts)
__device__ __forceinline__ float guided(float c, float u, float mc, float lc, float mu, float lu, float g) {
    const float a = (c - mc) - lc, w = (u - mu) - lu;
    return __builtin_fmaf(g, a - w, w);
}

__global__ __launch_bounds__(GD_THREADS) void guidance_lse_partial_kernel(const float *__restrict__ logits, int V, float *__restrict__ pval,
                                                                          float *__restrict__ psum) {
    __shared__ float s_v[GD_THREADS];
    __shared__ float s_s[GD_THREADS];
    const int b = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const float *row = logits + (int64_t)b * V;
    const int per = ((V + APART - 1) / APART + 3) & ~3;
    const int lo = min(V, part * per), hi = min(V, lo + per);
    float bv = -INFINITY, bs = 0.f;            // running maximum, sum of exp(l - bv): one exponential per value
    auto acc = [&](float v) {
        if (v > bv) { bs = bs * __expf(bv - v) + 1.f; bv = v; }
        else if (v > -INFINITY) bs += __expf(v - bv);
    };
    // thread t takes the groups of four ids lo + 4 (t + 256 k), in that order, then the t-th of the < 4 ids behind the last
    // group: which thread adds which id in which order depends on the ids alone.  Only the loads differ: one 16-byte load per
    // group where the part starts on a 16-byte boundary, four single loads of the same ids elsewhere.
    const int n4 = (hi - lo) >> 2;
    const bool vec = (reinterpret_cast<uintptr_t>(row + lo) & 15u) == 0;
    for (int q = tid; q < n4; q += GD_THREADS) {
        const int i = lo + 4 * q;
        float4 v;
        if (vec) v = *reinterpret_cast<const float4 *>(row + i);
        else v = make_float4(row[i], row[i + 1], row[i + 2], row[i + 3]);
        acc(v.x); acc(v.y); acc(v.z); acc(v.w);
    }
    if (tid < hi - (lo + 4 * n4)) acc(row[lo + 4 * n4 + tid]);
    s_v[tid] = bv;
    s_s[tid] = bs;
    __syncthreads();
    for (int o = GD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const float m = s_v[tid], v = s_v[tid + o], M = fmaxf(m, v);
            s_s[tid] = M == -INFINITY ? 0.f : s_s[tid] * __expf(m - M) + s_s[tid + o] * __expf(v - M);
            s_v[tid] = M;
        }
        __syncthreads();
    }
    if (tid == 0) {
        pval[b * APART + part] = s_v[0];
        psum[b * APART + part] = s_s[0];
    }
}

// logits [B, V] (rows need no alignment) -> pval / psum [B, APART]
hipError_t launch_guidance_lse_partial(const float *logits, int B, int V, float *pval, float *psum, hipStream_t s) {
    if (B < 1 || V < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guidance_lse_partial_kernel, dim3(APART, B), dim3(GD_THREADS), 0, s, logits, V, pval, psum);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void guidance_lse_final_kernel(const float *__restrict__ pval, const float *__restrict__ psum,
                                                                float *__restrict__ rmax, float *__restrict__ rlog,
                                                                float *__restrict__ rlse) {
    const int b = blockIdx.x, lane = threadIdx.x;
    static_assert(APART == 64, "one wave holds a row's parts");
    const float mp = pval[b * APART + lane], sp = psum[b * APART + lane];
    float M = mp;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    float e = mp > -INFINITY ? sp * expf(mp - M) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) {
        const float l = logf(e);
        rmax[b] = M;
        rlog[b] = l;
        rlse[b] = M + l;
    }
}

// pval / psum: launch_guidance_lse_partial's parts of B rows -> rmax, rlog, rlse [B]
hipError_t launch_guidance_lse_final(const float *pval, const float *psum, int B, float *rmax, float *rlog, float *rlse, hipStream_t s) {
    if (B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guidance_lse_final_kernel, dim3(B), dim3(64), 0, s, pval, psum, rmax, rlog, rlse);
    return hipGetLastError();
}

__global__ __launch_bounds__(GD_THREADS) void guidance_combine_kernel(float *__restrict__ cond, const float *__restrict__ uncond, int V,
                                                                      int chunk, const float *__restrict__ max_c,
                                                                      const float *__restrict__ log_c, const float *__restrict__ max_u,
                                                                      const float *__restrict__ log_u, const float *__restrict__ gp,
                                                                      float *__restrict__ keep) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = blockIdx.y * chunk, hi = min(V, lo + chunk);
    if (lo >= hi) return;
    float *rc = cond + (int64_t)b * V;
    const float *ru = uncond + (int64_t)b * V;
    float *rk = keep ? keep + (int64_t)b * V : nullptr;
    const float g = *gp, mc = max_c[b], lc = log_c[b], mu = max_u[b], lu = log_u[b];
    // ids whose address in the conditional row is 16-byte aligned are = r0 (mod 4)
    const unsigned pc = (unsigned)(reinterpret_cast<uintptr_t>(rc) & 15u);
    const int r0 = (int)(((16u - pc) & 15u) >> 2);
    const int i0 = min(hi, lo + ((r0 - lo) & 3));
    const int n4 = (hi - i0) >> 2;
    const bool u16 = (unsigned)(reinterpret_cast<uintptr_t>(ru) & 15u) == pc;
    const bool k16 = rk && (unsigned)(reinterpret_cast<uintptr_t>(rk) & 15u) == pc;
    if (tid < i0 - lo) {
        const int i = lo + tid;
        const float c = rc[i];
        if (rk) rk[i] = c;
        rc[i] = guided(c, ru[i], mc, lc, mu, lu, g);
    }
    for (int q = tid; q < n4; q += GD_THREADS) {
        const int i = i0 + 4 * q;
        const float4 c = *reinterpret_cast<const float4 *>(rc + i);
        float4 u;
        if (u16) u = *reinterpret_cast<const float4 *>(ru + i);
        else u = make_float4(ru[i], ru[i + 1], ru[i + 2], ru[i + 3]);
        if (rk) {
            if (k16) *reinterpret_cast<float4 *>(rk + i) = c;
            else { rk[i] = c.x; rk[i + 1] = c.y; rk[i + 2] = c.z; rk[i + 3] = c.w; }
        }
        *reinterpret_cast<float4 *>(rc + i) = make_float4(guided(c.x, u.x, mc, lc, mu, lu, g), guided(c.y, u.y, mc, lc, mu, lu, g),
                                                          guided(c.z, u.z, mc, lc, mu, lu, g), guided(c.w, u.w, mc, lc, mu, lu, g));
    }
    const int t0 = i0 + 4 * n4;
    if (tid < hi - t0) {
        const int i = t0 + tid;
        const float c = rc[i];
        if (rk) rk[i] = c;
        rc[i] = guided(c, ru[i], mc, lc, mu, lu, g);
    }
}

// cond / uncond: the first of n conditional rows and of their n partners (V floats each, any alignment); max_* / log_* [n]: the
// rows' maxima and log(sum exp(l - max)); g: one device float; keep: optional [n, V] copy of the raw conditional rows.
hipError_t launch_guidance_combine(float *cond, const float *uncond, int n, int V, const float *max_c, const float *log_c,
                                   const float *max_u, const float *log_u, const float *g, float *keep, hipStream_t s) {
    if (n < 1 || V < 1) return hipErrorInvalidValue;
    // about 1024 workgroups in all, none with less than 2048 ids (two passes of a workgroup's 16-byte accesses)
    int S = 1024 / n;
    const int most = (V + 2047) / 2048;
    S = S < 1 ? 1 : (S > most ? most : S);
    const int chunk = ((V + S - 1) / S + 3) & ~3;
    hipLaunchKernelGGL(guidance_combine_kernel, dim3(n, S), dim3(GD_THREADS), 0, s, cond, uncond, V, chunk, max_c, log_c, max_u, log_u, g, keep);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void guidance_pair_next_kernel(int32_t *__restrict__ next, int P) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < P) next[P + b] = next[b];
}

hipError_t launch_guidance_pair_next(int32_t *next, int P, hipStream_t s) {
    if (P < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guidance_pair_next_kernel, dim3((P + 63) / 64), dim3(64), 0, s, next, P);
    return hipGetLastError();
}

}  // namespace opus
