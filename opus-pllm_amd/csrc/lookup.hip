// Prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)): n-gram drafts from the row's own history, one verify pass of n
// positions per row, acceptance in lockstep.  The twin of every rule here is tests/lookup_ref.py.
//
//   lookup_draft_kernel   one workgroup per row.  The history of row b is hist[b, 0 .. hist_len[b]) (prompt ids, -1 where a protein
//                         block was spliced in, then -1 and the caller's corpus) followed by the gen ids generated so far
//                         (ids[b, 0 .. gen)).  Transformers' PromptLookupCandidateGenerator rule: for m from min(max_ngram, len - 1)
//                         down to 1 the FIRST window start i with h[i .. i + m) == h[len - m .. len) and a continuation
//                         (i + m < len, h[i + m] != -1) wins; the draft is h[i + m .. min(i + m + k, len)), cut in front of a -1.
//                         A tail that holds a -1 matches nothing (an equal window would hold it too).  Candidate starts are spread
//                         over the threads (start tid, tid + 256, ...: each thread stops at its first match, the lowest of its
//                         starts) and the minimum over the workgroup is taken through LDS, per m.  Writes draft[b, 0 .. k) (filler
//                         behind the draft), draft_len[b], optionally the row's last id in front of the draft (the verify pass's
//                         token matrix [R, k + 1]) and the longest draft of an unfinished row (atomicMax on a word the accept
//                         kernel zeroed).  A finished row drafts nothing.
//   lookup_embed_kernel   x[r n + j, :] = emb[tok[r, j]] in the operand type: the verify pass's input rows.
//   lookup_argmax_kernel  argmax_partial's parts -> one id per logits row (lowest index among ties, as the greedy step).
//   lookup_accept_kernel  ONE workgroup, thread b = row b (at most 64 rows).  y[b, j] = arg-max of row b at position j, x[b, j] the
//                         tokens that were fed (x[b, 0] the last committed token, x[b, 1 ..] the draft).
//                           m_b = the longest j <= draft_len[b] with x[b, i] == y[b, i - 1] for 1 <= i <= j
//                           a   = min of m_b over the rows that were unfinished when the pass began (LDS), cut to the id matrix
//                         Every row commits y[b, 0 .. a] at columns base .. base + a (base = step + pre): a finished row commits
//                         pad; an EOS id or the stop sequence among the COMMITTED ids finishes the row there, pad behind it.  The
//                         step word advances by pre (a + 1): a verify pass (pre = 1) appended a + 1 valid K / V slots, a plain
//                         decode step (pre = 0, n = 1) advanced the word itself.  n_unf[col] counts the rows still unfinished
//                         behind column col, as the greedy step does.  words = {a, rows unfinished, step word, ids drafted by
//                         unfinished rows}; the word for the next draft's maximum is zeroed.
#include "common.h"

namespace opus {

namespace {

constexpr int LK_THREADS = 256;
constexpr int LK_MAX_NGRAM = 8;

__global__ __launch_bounds__(LK_THREADS) void lookup_draft_kernel(const int32_t *__restrict__ hist, int ld_hist,
                                                                  const int32_t *__restrict__ hist_len, const int32_t *__restrict__ ids,
                                                                  int ld_ids, const int32_t *__restrict__ step, int gen_add,
                                                                  const int32_t *__restrict__ fin, int k, int max_ngram, int filler,
                                                                  int32_t *__restrict__ draft, int ld_draft, int32_t *__restrict__ first,
                                                                  int32_t *__restrict__ draft_len, int32_t *__restrict__ max_len) {
    __shared__ int s_min[LK_THREADS / 64];
    __shared__ int s_best;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L0 = hist_len ? hist_len[b] : 0;
    int gen = ids ? (step ? step[0] : 0) + gen_add : 0;
    gen = gen < 0 ? 0 : (gen > ld_ids ? ld_ids : gen);
    const int len = L0 + gen;
    const int32_t *hrow = hist + (int64_t)b * ld_hist, *grow = ids ? ids + (int64_t)b * ld_ids : hrow;
    auto h = [&](int i) { return i < L0 ? hrow[i] : grow[i - L0]; };
    const bool done = fin && fin[b];
    int32_t *drow = draft + (int64_t)b * ld_draft;
    if (first && tid == 0) first[(int64_t)b * ld_draft] = done || len < 1 ? filler : h(len - 1);
    int found = -1, fm = 0;
    if (!done) {
        const int m_hi = max_ngram < len - 1 ? max_ngram : len - 1;
        for (int m = m_hi; m >= 1; --m) {                       // (uniform over the workgroup)
            int tail[LK_MAX_NGRAM];
            bool ok = true;
#pragma unroll
            for (int j = 0; j < LK_MAX_NGRAM; ++j) {
                tail[j] = j < m ? h(len - m + j) : 0;
                ok = ok && (j >= m || tail[j] != -1);
            }
            int mine = 0x7fffffff;
            if (ok)
                for (int i = tid; i + m < len; i += LK_THREADS) {
                    bool eq = h(i + m) != -1;
#pragma unroll
                    for (int j = 0; j < LK_MAX_NGRAM; ++j) eq = eq && (j >= m || h(i + j) == tail[j]);
                    if (eq) { mine = i; break; }
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
            if ((tid & 63) == 0) s_min[tid >> 6] = mine;
            __syncthreads();
            if (tid == 0) {
                int v = s_min[0];
                for (int w = 1; w < LK_THREADS / 64; ++w) v = min(v, s_min[w]);
                s_best = v;
            }
            __syncthreads();
            const int best = s_best;
            __syncthreads();                                    // (s_min / s_best are written again by the next m)
            if (best != 0x7fffffff) { found = best; fm = m; break; }
        }
    }
    if (tid == 0) {
        int n = 0;
        if (found >= 0) {
            const int lo = found + fm, hi = lo + k < len ? lo + k : len;
            for (int i = lo; i < hi; ++i) {
                const int t = h(i);
                if (t == -1) break;
                drow[n++] = t;
            }
        }
        for (int j = n; j < k; ++j) drow[j] = filler;
        draft_len[b] = n;
        if (max_len && n > 0) atomicMax(max_len, n);
    }
}

__global__ __launch_bounds__(256) void lookup_embed_kernel(const int32_t *__restrict__ tok, int ld_tok, int n,
                                                           const half_t *__restrict__ emb, int H, int V, half_t *__restrict__ x) {
    const int row = blockIdx.x, r = row / n, j = row - r * n;
    int id = tok[(int64_t)r * ld_tok + j];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    for (int c = threadIdx.x; c < (H >> 3); c += 256)
        *reinterpret_cast<h8 *>(x + (int64_t)row * H + c * 8) = *reinterpret_cast<const h8 *>(emb + (int64_t)id * H + c * 8);
}

__global__ __launch_bounds__(64) void lookup_argmax_kernel(const float *__restrict__ pval, const int32_t *__restrict__ pidx,
                                                           int32_t *__restrict__ out) {
    static_assert(APART == 64, "one wave holds a row's parts");
    const int b = blockIdx.x, lane = threadIdx.x;
    float bv = pval[b * APART + lane];
    int bi = pidx[b * APART + lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(bv, o, 64);
        const int i = __shfl_xor(bi, o, 64);
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
    if (lane == 0) out[b] = bi == 0x7fffffff ? 0 : bi;
}

__global__ __launch_bounds__(64) void lookup_accept_kernel(LookupAcceptParams p) {
    __shared__ int s_a[64], s_unf[64], s_dr[64];
    const int b = threadIdx.x;
    const bool row = b < p.R;
    const int n = p.n, S = p.step[0], base = S + p.pre;
    int f = row && p.fin ? p.fin[b] : 0;
    int m = 0x7fffffff, dl = 0;
    if (row && !f) {
        dl = p.draft_len ? p.draft_len[b] : n - 1;
        dl = dl < 0 ? 0 : (dl > n - 1 ? n - 1 : dl);
        m = 0;
        while (m < dl && p.x[(int64_t)b * p.ld_x + m + 1] == p.y[(int64_t)b * n + m]) ++m;
    }
    s_a[b] = m;
    s_dr[b] = dl;
    __syncthreads();
    int a = 0x7fffffff, drafted = 0;
    for (int r = 0; r < 64; ++r) { a = min(a, s_a[r]); drafted += s_dr[r]; }
    if (a == 0x7fffffff) a = 0;                                 // (no unfinished row)
    if (p.ids) {                                                // the id matrix ends the chain
        const int room = p.stride - 1 - base;
        a = a > room ? room : a;
    }
    if (row && a >= 0) {
        int tok = p.pad;
        for (int j = 0; j <= a; ++j) {
            const int col = base + j;
            tok = f ? p.pad : p.y[(int64_t)b * n + j];
            if (p.ids) p.ids[(int64_t)b * p.stride + col] = tok;
            if (!f)
                for (int e = 0; e < p.n_eos; ++e) f |= (tok == p.eos[e]);
            if (!f && p.ids && p.n_stop > 0 && col + 1 >= p.n_stop) {
                bool hit = true;
                for (int q = 0; q < p.n_stop; ++q) hit = hit && p.ids[(int64_t)b * p.stride + col - p.n_stop + 1 + q] == p.stop[q];
                f |= hit ? 1 : 0;
            }
            if (!f && p.n_unf) atomicAdd(&p.n_unf[col], 1);
        }
        if (p.fin) p.fin[b] = f;
        if (p.next) p.next[b] = tok;
    }
    s_unf[b] = row && !f ? 1 : 0;
    __syncthreads();
    if (b == 0) {
        int unf = 0;
        for (int r = 0; r < 64; ++r) unf += s_unf[r];
        const int a_out = a < 0 ? 0 : a;
        const int S_new = S + (a >= 0 ? p.pre * (a + 1) : 0);
        p.step[0] = S_new;
        p.words[0] = a_out;
        p.words[1] = unf;
        p.words[2] = S_new;
        p.words[3] = drafted;
        if (p.max_len) *p.max_len = 0;
    }
}

}  // namespace

hipError_t launch_lookup_draft(const int32_t *hist, int ld_hist, const int32_t *hist_len, const int32_t *ids, int ld_ids,
                               const int32_t *step, int gen_add, const int32_t *fin, int R, int k, int max_ngram, int filler,
                               int32_t *draft, int ld_draft, int32_t *first, int32_t *draft_len, int32_t *max_len, hipStream_t s) {
    if (R < 1 || k < 1 || max_ngram < 1 || max_ngram > LK_MAX_NGRAM || ld_draft < k || !hist || !draft || !draft_len) return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, lookup_draft_kernel, dim3(R), dim3(LK_THREADS), 0, s, hist, ld_hist, hist_len, ids, ld_ids, step, gen_add, fin, k,
                max_ngram, filler, draft, ld_draft, first, draft_len, max_len);
    return hipGetLastError();
}

hipError_t launch_lookup_embed(const int32_t *tok, int ld_tok, int R, int n, const half_t *emb, int H, int V, half_t *x, hipStream_t s) {
    if (R < 1 || n < 1 || ld_tok < n || (H & 7)) return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, lookup_embed_kernel, dim3(R * n), dim3(256), 0, s, tok, ld_tok, n, emb, H, V, x);
    return hipGetLastError();
}

hipError_t launch_lookup_argmax(const float *pval, const int32_t *pidx, int rows, int32_t *out, hipStream_t s) {
    if (rows < 1) return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, lookup_argmax_kernel, dim3(rows), dim3(64), 0, s, pval, pidx, out);
    return hipGetLastError();
}

hipError_t launch_lookup_accept(const LookupAcceptParams &p, hipStream_t s) {
    if (p.R < 1 || p.R > 64 || p.n < 1 || p.ld_x < p.n || p.n_stop < 0 || p.n_stop > 8 || p.n_eos < 0 || p.n_eos > 64 || !p.y || !p.x ||
        !p.step || !p.words || (p.pre != 0 && p.pre != 1) || (p.pre == 0 && p.n != 1))
        return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, lookup_accept_kernel, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

int lookup_max_ngram() { return LK_MAX_NGRAM; }

}  // namespace opus
