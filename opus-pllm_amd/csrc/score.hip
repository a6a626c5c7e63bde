// Teacher-forced scoring (opus_llama_forward): the row gather in front of the lm_head over many rows and the log-softmax /
// NLL reduction behind it.
//   gather_rows : out[r] = x[rows[r]] for fp32 residual-stream rows (launch_take_last with an index list); gather_rows2 the
//                 same over two sources (opus_llama_score_continuations: continuation rows and the prefix's last rows)
//   xent        : per row of operand-dtype logits [R, V] and target y: lse = logsumexp(l), logprob = l[y] - lse (fp32)
#include "common.h"

namespace opus {

// One workgroup per gathered row, float4 copies (H % 4 == 0).  An index outside [0, n_src) yields a zero row: nothing is read
// out of bounds whatever the caller passed.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ x, const int32_t *__restrict__ rows,
                                                          int64_t n_src, int H, float *__restrict__ out) {
    const int r = blockIdx.x;
    const int64_t src = rows[r];
    float4 *dst = reinterpret_cast<float4 *>(out + (int64_t)r * H);
    if (src < 0 || src >= n_src) {
        for (int c = threadIdx.x; c < (H >> 2); c += 256) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4 *s = reinterpret_cast<const float4 *>(x + src * H);
    for (int c = threadIdx.x; c < (H >> 2); c += 256) dst[c] = s[c];
}
hipError_t launch_gather_rows(const float *x, const int32_t *rows, int R, int64_t n_src, int H, float *out, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (H & 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(R), dim3(256), 0, s, x, rows, n_src, H, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gather_rows2_kernel(const float *__restrict__ x, int64_t n_x, const float *__restrict__ y,
                                                           int64_t n_y, const int32_t *__restrict__ rows, int H,
                                                           float *__restrict__ out) {
    const int r = blockIdx.x;
    const int64_t i = rows[r];
    const float *src = i >= 0 ? (i < n_x ? x + i * H : nullptr) : (-i - 1 < n_y ? y + (-i - 1) * H : nullptr);
    float4 *dst = reinterpret_cast<float4 *>(out + (int64_t)r * H);
    for (int c = threadIdx.x; c < (H >> 2); c += 256)
        dst[c] = src ? reinterpret_cast<const float4 *>(src)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}
hipError_t launch_gather_rows2(const float *x, int64_t n_x, const float *y, int64_t n_y, const int32_t *rows, int R, int H, float *out,
                               hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (H & 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows2_kernel, dim3(R), dim3(256), 0, s, x, n_x, y, n_y, rows, H, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ log-softmax / NLL
// Online (max, sum-exp) pairs.  A running max of -inf (nothing seen, or only -inf logits) is rebased at 0 so that exp() never
// sees -inf - (-inf).
struct MS {
    float m, s;
};
__device__ __forceinline__ float safe_base(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ MS ms_merge(MS a, MS b) {
    const float m = fmaxf(a.m, b.m), base = safe_base(m);
    return MS{m, a.s * __expf(a.m - base) + b.s * __expf(b.m - base)};
}
__device__ __forceinline__ void ms_add1(MS &a, float v) {
    if (v > a.m) {
        a.s *= __expf(a.m - v);
        a.m = v;
    }
    a.s += __expf(v - safe_base(a.m));
}
__device__ __forceinline__ void ms_add8(MS &a, const h8 v) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
    const float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
    if (mx > a.m) {
        a.s *= __expf(a.m - mx);
        a.m = mx;
    }
    const float base = safe_base(a.m);
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) e += __expf(f[j] - base);
    a.s += e;
}

// WPR waves per row (4: one row per workgroup; 1: four rows per workgroup, small V).  Every lane walks its own 16-byte vectors of
// the row (8 logits per load, UNR loads in flight) with an fp32 online max / sum-exp; the scalar head up to the first 16-byte
// boundary and the tail after the last whole vector (V % 8 != 0, or a row that does not start on a boundary) go to the first
// lanes.  The lanes' pairs are merged by a 64-lane butterfly and then across the waves in LDS in wave order: a fixed reduction
// order, no atomics, so the same logits give bitwise the same outputs.
template <int WPR>
__global__ __launch_bounds__(256) void xent_kernel(const half_t *__restrict__ logits, int64_t ld, int R, int V,
                                                   const int32_t *__restrict__ targets, float *__restrict__ logprob,
                                                   float *__restrict__ lse_out) {
    constexpr int P = WPR * 64, UNR = 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = WPR == 4 ? blockIdx.x : blockIdx.x * 4 + wave;
    const int t = WPR == 4 ? threadIdx.x : lane;
    if (row >= R) return;                                    // (WPR == 1: whole waves leave; no barrier below in that case)
    const half_t *p = logits + (int64_t)row * ld;
    const int head = min((int)(((16 - ((uintptr_t)p & 15)) & 15) >> 1), V);
    const int nvec = (V - head) >> 3;
    const int tail0 = head + nvec * 8;
    const h8 *pv = reinterpret_cast<const h8 *>(p + head);
    MS a{-INFINITY, 0.f};
    if (t < head) ms_add1(a, (float)p[t]);
    if (t < V - tail0) ms_add1(a, (float)p[tail0 + t]);
    h8 ninf;
#pragma unroll
    for (int j = 0; j < 8; ++j) ninf[j] = (half_t)(-INFINITY);
    for (int i0 = t; i0 < nvec; i0 += UNR * P) {
        h8 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = i0 + u * P < nvec ? pv[i0 + u * P] : ninf;
#pragma unroll
        for (int u = 0; u < UNR; ++u) ms_add8(a, v[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const MS b{__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)};
        a = ms_merge(a, b);
    }
    if (WPR > 1) {
        __shared__ MS part[4];
        if (lane == 0) part[wave] = a;
        __syncthreads();
        if (threadIdx.x != 0) return;
        a = part[0];
#pragma unroll
        for (int w = 1; w < WPR; ++w) a = ms_merge(a, part[w]);
    } else if (lane != 0) {
        return;
    }
    const float logs = __logf(a.s);
    if (lse_out) lse_out[row] = a.m + logs;
    const int y = targets[row];
    float lp;
    if (y < 0) lp = 0.f;                                      // not a counted target (ignore_index): contributes nothing
    else if (y >= V) lp = __builtin_nanf("");
    else lp = ((float)p[y] - a.m) - logs;                     // (l[y] - max is exact in fp32: no cancellation against lse)
    logprob[row] = lp;
}

hipError_t launch_xent(const half_t *logits, int64_t ld, int R, int V, const int32_t *targets, float *logprob, float *lse,
                       hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (V < 1 || ld < V) return hipErrorInvalidValue;
    if (V >= 4096) hipLaunchKernelGGL(xent_kernel<4>, dim3(R), dim3(256), 0, s, logits, ld, R, V, targets, logprob, lse);
    else hipLaunchKernelGGL(xent_kernel<1>, dim3((R + 3) / 4), dim3(256), 0, s, logits, ld, R, V, targets, logprob, lse);
    return hipGetLastError();
}

}  // namespace opus
