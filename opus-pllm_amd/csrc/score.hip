// Teacher-forced scoring (opus_llama_forward): the row gather in front of the lm_head over many rows and the log-softmax /
// NLL reduction behind it.
//   gather_rows : out[r] = x[rows[r]] for fp32 residual-stream rows (launch_take_last with an index list); gather_rows2 the
//                 same over two sources (opus_llama_score_continuations: continuation rows and the prefix's last rows)
//   xent        : per row of operand-dtype logits [R, V] and target y: lse = logsumexp(l), logprob = l[y] - lse (fp32)
//   tree_edges  : trie scoring (opus_llama_score_tree): many (row, token) edges and stop-id sums read from one chunk of logits
//   tree_path_sums : a member's log-prob = the sum of its path's node log-probs (opus_trie_path_sums)
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

// ------------------------------------------------------------------------------ trie scoring
// A thread per edge, then a thread per stop entry.  Every output slot is written by exactly one thread and every sum runs in list
// order: no atomics, bitwise repeatable.
__global__ __launch_bounds__(256) void tree_edges_kernel(const half_t *__restrict__ logits, int64_t ld, const float *__restrict__ lse,
                                                         int row0, const int32_t *__restrict__ erow, const int32_t *__restrict__ etok,
                                                         const int32_t *__restrict__ eslot, int n_edges, float *__restrict__ node_lp,
                                                         const int32_t *__restrict__ srow, const int32_t *__restrict__ sset,
                                                         const int32_t *__restrict__ sslot, int n_stops,
                                                         const int32_t *__restrict__ ids, const int32_t *__restrict__ soff,
                                                         float *__restrict__ stop_lp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_edges) {
        const int r = erow[i] - row0;
        node_lp[eslot[i]] = (float)logits[(int64_t)r * ld + etok[i]] - lse[r];
    } else if (i < n_edges + n_stops) {
        const int k = i - n_edges, r = srow[k] - row0, set = sset[k];
        const half_t *p = logits + (int64_t)r * ld;
        const float base = lse[r];
        float sum = 0.f;
        for (int j = soff[set]; j < soff[set + 1]; ++j) sum += __expf((float)p[ids[j]] - base);
        stop_lp[sslot[k]] = __logf(sum);
    }
}
hipError_t launch_tree_edges(const half_t *logits, int64_t ld, const float *lse, int row0, const int32_t *erow, const int32_t *etok,
                             const int32_t *eslot, int n_edges, float *node_lp, const int32_t *srow, const int32_t *sset,
                             const int32_t *sslot, int n_stops, const int32_t *ids, const int32_t *soff, float *stop_lp, hipStream_t s) {
    const int n = n_edges + n_stops;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tree_edges_kernel, dim3((n + 255) / 256), dim3(256), 0, s, logits, ld, lse, row0, erow, etok, eslot, n_edges,
                       node_lp, srow, sset, sslot, n_stops, ids, soff, stop_lp);
    return hipGetLastError();
}

// A thread per (prefix row, member).  The path is added root to leaf: step k re-walks the parent chain from the member's node to
// its ancestor at depth k + 1 (depth^2 / 2 table reads for a path of a few tokens; no per-thread array, so no scratch memory).
__global__ __launch_bounds__(256) void tree_path_sums_kernel(const float *__restrict__ node_lp, const int32_t *__restrict__ trie,
                                                             const int32_t *__restrict__ par, const int32_t *__restrict__ depth,
                                                             const int32_t *__restrict__ mnode, int P, int M, int ld_nodes,
                                                             float *__restrict__ member_lp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)P * M) return;
    const int p = (int)(i / M), m = (int)(i - (int64_t)p * M);
    const int t = trie[p];
    const int leaf = mnode[(int64_t)t * M + m];
    if (leaf < 0) {
        member_lp[i] = -INFINITY;
        return;
    }
    const int32_t *pa = par + (int64_t)t * ld_nodes;
    const float *lp = node_lp + (int64_t)p * ld_nodes;
    const int d = depth[(int64_t)t * ld_nodes + leaf];
    float sum = 0.f;
    for (int k = 1; k <= d; ++k) {
        int v = leaf;
        for (int up = d - k; up > 0; --up) v = pa[v];
        sum += lp[v];
    }
    member_lp[i] = sum;
}
hipError_t launch_tree_path_sums(const float *node_lp, const int32_t *trie, const int32_t *par, const int32_t *depth,
                                 const int32_t *mnode, int P, int M, int ld_nodes, float *member_lp, hipStream_t s) {
    if (P <= 0 || M <= 0) return hipSuccess;
    const int64_t n = (int64_t)P * M;
    hipLaunchKernelGGL(tree_path_sums_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, node_lp, trie, par, depth, mnode, P,
                       M, ld_nodes, member_lp);
    return hipGetLastError();
}

}  // namespace opus
