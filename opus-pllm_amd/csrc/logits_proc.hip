// generate()'s logits processors (transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
// NoBadWordsLogitsProcessor, MinLengthLogitsProcessor / MinNewTokensLengthLogitsProcessor, in that order), applied in place to
// the fp32 logits of a decode step before the arg-max or the sampling head reads them.
//
// History: the ids generated so far, row b's at hist[b * ld + 0 .. t), t = *step (the device step word: a captured step serves
// every call).  The reference generates from inputs_embeds, so transformers starts input_ids empty and no processor ever sees the
// prompt; a finished row's history holds its pad ids, as in transformers.
//
// One workgroup per row; the edits are sparse (at most t + n_bad + n_eos entries) and the kernel never sweeps the vocabulary.
//   phase 1  repetition penalty, s < 0 ? s * p : s / p, once per distinct history id: every history position reads its raw
//            logit first (and records it in raw_hist when the caller wants the raw values back); after a barrier the first
//            occurrence of each id writes the penalised value - a later duplicate never reads a penalised one.
//   phase 2  (after a barrier, so that no penalty write can land on top of a ban) -inf for the id behind every earlier
//            occurrence of the last n - 1 ids, for bad-word ends whose prefix the history ends with, and for the EOS ids while
//            t < min_new.
// The division is IEEE fp32 (no fast-math in build.py): bit-exact to torch's `scores / penalty`.
#include "common.h"

namespace opus {

__global__ __launch_bounds__(256) void logits_proc_kernel(float *__restrict__ logits, int V, const int32_t *__restrict__ hist,
                                                          int64_t ld, const int32_t *__restrict__ step, int max_hist,
                                                          const int32_t *__restrict__ eos, int n_eos,
                                                          const LogitsProcDesc *__restrict__ d, float *__restrict__ raw_hist) {
    __shared__ int32_t s_h[LP_MAX_HIST];
    __shared__ float s_p[LP_MAX_HIST];
    const int b = blockIdx.x, tid = threadIdx.x;
    float *row = logits + (int64_t)b * V;
    const int32_t *h = hist + (int64_t)b * ld;
    int t = *step;
    t = t < 0 ? 0 : (t > max_hist ? max_hist : t);
    const float pen = d->penalty;
    const int ngram = d->ngram, min_new = d->min_new, n_bad = d->n_bad;
    for (int i = tid; i < t; i += 256) s_h[i] = h[i];
    __syncthreads();

    // phase 1: read every history id's raw logit, then penalise each distinct id once
    const bool penal = pen != 1.0f;
    if (penal || raw_hist) {
        for (int i = tid; i < t; i += 256) {
            const int id = s_h[i];
            const float raw = (unsigned)id < (unsigned)V ? row[id] : 0.f;
            if (raw_hist) raw_hist[(int64_t)b * ld + i] = raw;
            s_p[i] = raw < 0.f ? raw * pen : raw / pen;
        }
        __syncthreads();
        if (penal)
            for (int i = tid; i < t; i += 256) {
                const int id = s_h[i];
                bool first = (unsigned)id < (unsigned)V;
                for (int j = 0; j < i && first; ++j) first = s_h[j] != id;
                if (first) row[id] = s_p[i];
            }
    }
    __syncthreads();

    // phase 2: bans
    if (ngram > 0 && t + 1 >= ngram) {
        const int tail = t - ngram + 1;                   // the last n - 1 ids start here
        for (int i = tid; i <= t - ngram; i += 256) {     // the n-gram at i: prefix s_h[i .. i + n - 2], then s_h[i + n - 1]
            bool hit = true;
            for (int k = 0; k < ngram - 1 && hit; ++k) hit = s_h[i + k] == s_h[tail + k];
            const int id = s_h[i + ngram - 1];
            if (hit && (unsigned)id < (unsigned)V) row[id] = -INFINITY;
        }
    }
    for (int e = tid; e < n_bad; e += 256) {
        const int o = d->bad_off[e], L = d->bad_off[e + 1] - o;
        const int last = d->bad_ids[o + L - 1];
        bool hit;
        if (L == 1) {                                     // a single id equal to an EOS id is dropped (transformers' filter)
            hit = true;
            for (int k = 0; k < n_eos; ++k) hit = hit && eos[k] != last;
        } else {                                          // (transformers skips an entry longer than the history: t >= L)
            hit = t >= L;
            for (int k = 0; k < L - 1 && hit; ++k) hit = s_h[t - L + 1 + k] == d->bad_ids[o + k];
        }
        if (hit && (unsigned)last < (unsigned)V) row[last] = -INFINITY;
    }
    if (t < min_new)
        for (int k = tid; k < n_eos; k += 256)
            if ((unsigned)eos[k] < (unsigned)V) row[eos[k]] = -INFINITY;
}

hipError_t launch_logits_proc(float *logits, int B, int V, const int32_t *hist, int64_t ld, const int32_t *step, int max_hist,
                              const int32_t *eos, int n_eos, const LogitsProcDesc *desc, float *raw_hist, hipStream_t s) {
    if (max_hist > LP_MAX_HIST) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logits_proc_kernel, dim3(B), dim3(256), 0, s, logits, V, hist, ld, step, max_hist, eos, n_eos, desc, raw_hist);
    return hipGetLastError();
}

}  // namespace opus
