// generate(top_logprobs=k) / forward(labels, top_logprobs=k): the k likeliest tokens of a logits row and their log-probabilities.
//
// Order: value descending, then index ascending (np.argsort(-l, kind="stable")[:k]).  One 64-bit key per entry carries it: the
// monotone uint32 image of the float in the high word (-0 counted as +0, so that equal values have equal images), ~index in the
// low word.  Keys of a row are distinct, a plain unsigned maximum picks the lower index among equal values, and "the best key
// below the last winner" is the next entry of the order - nothing is removed, nothing is held in indexed registers (no scratch).
// Key 0 is padding: the image of -inf is 0x007fffff, so padding loses to every real entry.
//
//   topk_part_kernel<T>  grid (APART parts, rows), the part cut of argmax_lse_partial_kernel (per, lo, hi): k rounds, each a block
//                        maximum over the part's keys below the previous round's winner (the part is re-read: at most a few KB,
//                        from the cache); round j's winner goes to cand[row, part, j], 0 once the part is exhausted.
//   topk_merge_kernel<T> one wave per row, lane p holding part p's k candidates in registers (unrolled to TOPK_MAX): k rounds of a
//                        wave maximum below the last winner, lane j keeping winner j; then lanes 0 .. k-1 write
//                        ids[row, step, j] and l[id] - lse.  The lse is the caller's (lse_in[row]) or, from argmax_lse_partial's
//                        parts, bitwise argmax_lse_step_kernel's: the same butterfly maximum and parts_lse.
//   topk_row_lse_kernel<T>  opus_debug_top_logprobs without an lse on rows argmax_lse_partial cannot take (16-bit, or a leading
//                        dimension): one block per row, maximum then sum.
#include "common.h"

namespace opus {

static __device__ __forceinline__ uint32_t f32_image(float v) {
    if (v == 0.f) v = 0.f;                                    // -0 -> +0
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
static __device__ __forceinline__ uint64_t topk_key(float v, int i) { return ((uint64_t)f32_image(v) << 32) | (uint32_t)~(uint32_t)i; }
static __device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(x >> 32), o, 64), lo = __shfl_xor((uint32_t)x, o, 64);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}

template <typename T>
__global__ __launch_bounds__(256) void topk_part_kernel(const T *__restrict__ logits, int64_t ld, int V, const GenOutDesc *__restrict__ desc,
                                                        int k_arg, uint64_t *__restrict__ cand) {
    __shared__ uint64_t s_w[2][4];
    const int b = blockIdx.y, part = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = min(desc ? desc->top_k : k_arg, TOPK_MAX);
    const T *row = logits + (int64_t)b * ld;
    const int per = ((V + APART - 1) / APART + 3) & ~3;
    const int lo = part * per, hi = (lo + per < V ? lo + per : (lo < V ? V : lo));
    uint64_t *out = cand + ((int64_t)b * APART + part) * TOPK_MAX;
    uint64_t prev = ~0ull;
    for (int j = 0; j < k; ++j) {                             // (k is uniform: every thread reaches every barrier)
        uint64_t best = 0;
        for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
            const uint64_t key = topk_key((float)row[i], i);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        if (lane == 0) s_w[j & 1][wave] = best;
        __syncthreads();                                      // (one barrier a round: round j + 2 rewrites what round j read only
        const uint64_t a = s_w[j & 1][0], c = s_w[j & 1][1], d = s_w[j & 1][2], e = s_w[j & 1][3];   //  after round j + 1's barrier)
        const uint64_t ac = a > c ? a : c, de = d > e ? d : e;
        prev = ac > de ? ac : de;
        if (threadIdx.x == 0) out[j] = prev;
        if (prev == 0) {                                      // the part is exhausted (uniform): the rest is padding
            for (int q = j + 1 + (int)threadIdx.x; q < k; q += 256) out[q] = 0;
            break;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void topk_merge_kernel(const T *__restrict__ logits, int64_t ld, int V, const uint64_t *__restrict__ cand,
                                                        const float *__restrict__ lse_in, const float *__restrict__ pval,
                                                        const float *__restrict__ psum, const int32_t *__restrict__ finished,
                                                        const int32_t *__restrict__ step, int max_new,
                                                        const GenOutDesc *__restrict__ desc, int k_arg, int32_t *__restrict__ ids_arg,
                                                        float *__restrict__ lp_arg) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int k = min(desc ? desc->top_k : k_arg, TOPK_MAX);
    int32_t *ids = desc ? desc->top_ids : ids_arg;
    float *lps = desc ? desc->top_lp : lp_arg;
    const int st = step ? *step : 0;
    if (st >= max_new) return;
    const int64_t o = ((int64_t)b * max_new + st) * k;
    if (finished && finished[b]) {                            // the row had finished before this step
        if (lane < k) { ids[o + lane] = -1; lps[o + lane] = 0.f; }
        return;
    }
    float lse;
    if (lse_in) {
        lse = lse_in[b];
    } else {                                                  // argmax_lse_step_kernel's arithmetic
        static_assert(APART == 64, "one wave holds a row's parts");
        const float mp = pval[b * APART + lane], sp = psum[b * APART + lane];
        float M = mp;
#pragma unroll
        for (int q = 32; q > 0; q >>= 1) M = fmaxf(M, __shfl_xor(M, q, 64));
        float e = mp > -INFINITY ? sp * __expf(mp - M) : 0.f;
#pragma unroll
        for (int q = 32; q > 0; q >>= 1) e += __shfl_xor(e, q, 64);
        lse = M + logf(e);
    }
    const uint64_t *mine = cand + ((int64_t)b * APART + lane) * TOPK_MAX;
    uint64_t c[TOPK_MAX];
#pragma unroll
    for (int j = 0; j < TOPK_MAX; ++j) c[j] = j < k ? mine[j] : 0;
    uint64_t prev = ~0ull, won = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t best = 0;
#pragma unroll
        for (int q = 0; q < TOPK_MAX; ++q)
            if (c[q] < prev && c[q] > best) best = c[q];
        prev = wave_max_u64(best);
        if (lane == j) won = prev;
    }
    if (lane < k) {
        const int id = (int)~(uint32_t)won;
        const bool real = won != 0 && (unsigned)id < (unsigned)V;          // (k <= V: always; a stray key must not index the row)
        ids[o + lane] = real ? id : -1;
        lps[o + lane] = real ? (float)logits[(int64_t)b * ld + id] - lse : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void topk_row_lse_kernel(const T *__restrict__ logits, int64_t ld, int V, float *__restrict__ lse) {
    __shared__ float s_f[4];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T *row = logits + (int64_t)b * ld;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, (float)row[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_f[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
    __syncthreads();
    float e = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) {
        const float v = (float)row[i];
        if (v > -INFINITY) e += __expf(v - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) s_f[wave] = e;
    __syncthreads();
    if (threadIdx.x == 0) lse[b] = m + logf((s_f[0] + s_f[1]) + (s_f[2] + s_f[3]));
}

template <typename T>
static hipError_t topk_launch(const T *logits, int64_t ld, int R, int V, const TopkArgs &a, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (V < 1 || ld < V || !a.cand || (!a.desc && (a.k < 1 || a.k > TOPK_MAX || a.k > V || !a.ids || !a.lp)) ||
        (!a.lse && !(a.pval && a.psum)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_part_kernel<T>, dim3(APART, R), dim3(256), 0, s, logits, ld, V, a.desc, a.k, a.cand);
    hipLaunchKernelGGL(topk_merge_kernel<T>, dim3(R), dim3(64), 0, s, logits, ld, V, a.cand, a.lse, a.pval, a.psum, a.finished, a.step,
                       a.step ? a.max_new : 1, a.desc, a.k, a.ids, a.lp);
    return hipGetLastError();
}
hipError_t launch_topk_f32(const float *logits, int64_t ld, int R, int V, const TopkArgs &a, hipStream_t s) {
    return topk_launch(logits, ld, R, V, a, s);
}
hipError_t launch_topk_h16(const half_t *logits, int64_t ld, int R, int V, const TopkArgs &a, hipStream_t s) {
    return topk_launch(logits, ld, R, V, a, s);
}
hipError_t launch_topk_row_lse(const void *logits, bool f32, int64_t ld, int R, int V, float *lse, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (f32) hipLaunchKernelGGL(topk_row_lse_kernel<float>, dim3(R), dim3(256), 0, s, (const float *)logits, ld, V, lse);
    else hipLaunchKernelGGL(topk_row_lse_kernel<half_t>, dim3(R), dim3(256), 0, s, (const half_t *)logits, ld, V, lse);
    return hipGetLastError();
}

}  // namespace opus
