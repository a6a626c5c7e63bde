// Continuous batching (opus_stream_*): the small device work around a decode batch whose finished rows are handed to new prompts.
//
// A session's step t writes every row's token to column t of the id buffer [B, S] and its K / V to cache slot T0 + t.  A row r is
// occupied from step start[r] on; it is done at the first step end[r] at which the step kernel marked it finished (EOS id, stop
// sequence) or its budget of max_new tokens is used up.
//
// stream_finish_kernel runs behind the step kernel of every step: budget, end[], the count of rows not done (poll[B], beside the
// end steps poll[0 .. B) the host copies out per step).  stream_refill_kernel runs at a step boundary behind kv_place_kernel: it
// makes the listed rows the new prompts' rows - last-position logits, kstart, start, the cleared flags, and -1 in the id columns
// the stop-sequence test of the next steps reads back into (so that it never matches the previous occupant's tail).
#include "common.h"

namespace opus {

namespace {

// one workgroup, rows strided over its threads
__global__ __launch_bounds__(256) void stream_finish_kernel(const int32_t *__restrict__ step, const int32_t *__restrict__ start,
                                                            int32_t *__restrict__ fin, int32_t *__restrict__ poll, int B, int max_new) {
    __shared__ int live;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    const int t = step[0];
    int mine = 0;
    for (int r = threadIdx.x; r < B; r += 256) {
        int done = fin[r];
        if (!done && t + 1 - start[r] >= max_new) {
            done = 1;
            fin[r] = 1;                                            // the row emits pad ids from the next step on
        }
        if (done && poll[r] < 0) poll[r] = t;
        mine += done ? 0 : 1;
    }
    if (mine) atomicAdd(&live, mine);
    __syncthreads();
    if (threadIdx.x == 0) poll[B] = live;
}

// grid (listed rows, column blocks): listed row i = decode row rows[i], its logits from row src[i] of `logits_in`
__global__ __launch_bounds__(256) void stream_refill_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ src,
                                                            const int32_t *__restrict__ nks, const float *__restrict__ logits_in,
                                                            float *__restrict__ logits, int V, int32_t *__restrict__ kstart,
                                                            int32_t *__restrict__ start, int32_t *__restrict__ fin,
                                                            int32_t *__restrict__ poll, int32_t *__restrict__ ids, int S, int t) {
    const int r = rows[blockIdx.x], tid = threadIdx.x;
    const float *in = logits_in + (int64_t)src[blockIdx.x] * V;
    float *out = logits + (int64_t)r * V;
    if ((V & 3) == 0) {                                            // (both bases are 16-byte aligned: rows stay so when V % 4 == 0)
        for (int i = blockIdx.y * 256 + tid; i < (V >> 2); i += gridDim.y * 256)
            reinterpret_cast<float4 *>(out)[i] = reinterpret_cast<const float4 *>(in)[i];
    } else {
        for (int i = blockIdx.y * 256 + tid; i < V; i += gridDim.y * 256) out[i] = in[i];
    }
    if (blockIdx.y != 0) return;
    if (tid == 0) {
        kstart[r] = nks[r];
        start[r] = t;
        fin[r] = 0;
        poll[r] = -1;
    }
    if (tid < 8 && t - 8 + tid >= 0) ids[(int64_t)r * S + t - 8 + tid] = -1;
}

// start[r] = 0, end[r] = -1 for the rows of a new session; poll[B] = B
__global__ __launch_bounds__(256) void stream_reset_kernel(int32_t *__restrict__ start, int32_t *__restrict__ poll, int B) {
    for (int r = threadIdx.x; r < B; r += 256) {
        start[r] = 0;
        poll[r] = -1;
    }
    if (threadIdx.x == 0) poll[B] = B;
}

}  // namespace

hipError_t launch_stream_finish(const int32_t *step, const int32_t *start, int32_t *fin, int32_t *poll, int B, int max_new, hipStream_t s) {
    if (B < 1 || max_new < 1) return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, stream_finish_kernel, dim3(1), dim3(256), 0, s, step, start, fin, poll, B, max_new);
    return hipGetLastError();
}

hipError_t launch_stream_refill(const int32_t *rows, const int32_t *src, const int32_t *nks, int n, const float *logits_in, float *logits,
                                int V, int32_t *kstart, int32_t *start, int32_t *fin, int32_t *poll, int32_t *ids, int S, int t,
                                hipStream_t s) {
    if (n < 1 || V < 1 || S < 1 || t < 0 || t >= S || logits_in == logits) return hipErrorInvalidValue;
    const int gy = (int)cdiv(cdiv(V, 4), 256);
    OPUS_LAUNCH(KC_OTHER, stream_refill_kernel, dim3(n, gy > 64 ? 64 : gy), dim3(256), 0, s, rows, src, nks, logits_in, logits, V, kstart,
                start, fin, poll, ids, S, t);
    return hipGetLastError();
}

hipError_t launch_stream_reset(int32_t *start, int32_t *poll, int B, hipStream_t s) {
    if (B < 1) return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, stream_reset_kernel, dim3(1), dim3(256), 0, s, start, poll, B);
    return hipGetLastError();
}

}  // namespace opus
