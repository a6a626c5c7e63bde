// Trie search (OpusLlamaForCausalLM.search_trie): beam search for the best members of a TokenTrie behind a cached prefix.  The
// decoder runs P x K rows (row = p K + k) through opus_llama_prefill_behind / opus_llama_decode_step; between two passes ONE
// launch of trie_beam_expand_kernel does everything a level needs, one workgroup per prompt, so the host keeps no per-beam
// bookkeeping: it feeds `parent` to opus_kv_reorder, `tok` to the next step and reads trie_search_summary_kernel's two words.
//
// The table (opus_set_trie_search) is the tries' children in CSR form: state s owns the edges edge_off[s] .. edge_off[s + 1)
// (ids ascending, edge_next the child states), member[s] is the member index of a state that completes a member (-1 otherwise)
// and stop_set[s] the id set of its trie (stop_off / stop_ids: the end ids, then the separator's first id).  State 0 is the dead
// state: no edges, no member.
//
// A level, for prompt p with beams (state, run) k = 0 .. K - 1 whose logits rows and log-sum-exp are given (dead beams: state 0 or
// run = -inf, never read):
//   1. pool    include_stop: every live beam on a member state offers (member, run, stop = log sum_{i in set} exp(l[i] - lse)) to
//              the pool; otherwise every child that is a member offers (member, run + (l[tok] - lse)).  The pool keeps the best
//              `top` by lp + stop descending, ties to the lower member index.
//   2. beams   every child of a live beam (without include_stop: every child that has a child) competes with
//              run + (l[tok] - lse) for the K slots: descending, ties to the lower (beam, id).  More competitors than slots clear
//              the prompt's `exhaustive` word.
//   3. stop    no live beam left, or the best one strictly below the pool's top-th entry: the prompt stops (all beams dead).
// Only the allowed entries of the logits are read, nothing is written to them.  Selection is beam_topk_kernel's: per-thread
// sorted lists in registers (static indices), then block arg-max rounds over a fixed tree; all sums run in list order: bitwise
// repeatable.  Every loop is bounded by K, top, the state's edge count or the set's size.
#include "common.h"

namespace opus {

static constexpr int TS_NONE = 0x7fffffff;

// candidate (s, i) into the sorted list bs / bi (descending, ties to the lower i); static indices: the list stays in registers
__device__ __forceinline__ void ts_insert(float (&bs)[TS_MAXK], int (&bi)[TS_MAXK], float sc, int id) {
    if (sc > bs[TS_MAXK - 1] || (sc == bs[TS_MAXK - 1] && id < bi[TS_MAXK - 1])) {
        float cs = sc;
        int ci = id;
#pragma unroll
        for (int j = 0; j < TS_MAXK; ++j) {
            const bool better = cs > bs[j] || (cs == bs[j] && ci < bi[j]);
            const float ts = better ? bs[j] : cs;
            const int ti = better ? bi[j] : ci;
            bs[j] = better ? cs : bs[j];
            bi[j] = better ? ci : bi[j];
            cs = ts;
            ci = ti;
        }
    }
}

// `rounds` block arg-max rounds over the heads of the threads' lists -> sel_s / sel_i [rounds] (-inf / TS_NONE behind the last
// candidate).  Ends with a barrier.
__device__ __forceinline__ void ts_select(const float (&bs)[TS_MAXK], const int (&bi)[TS_MAXK], int rounds, float *s_v, int *s_i,
                                          int *s_who, float *sel_s, int *sel_i) {
    const int tid = threadIdx.x;
    int head = 0;
    for (int r = 0; r < rounds; ++r) {
        float hv = -INFINITY;
        int hi = TS_NONE;
#pragma unroll
        for (int j = 0; j < TS_MAXK; ++j)
            if (j == head) { hv = bs[j]; hi = bi[j]; }
        s_v[tid] = hv; s_i[tid] = hi; s_who[tid] = tid;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                const float v = s_v[tid + o];
                const int i = s_i[tid + o];
                if (v > s_v[tid] || (v == s_v[tid] && i < s_i[tid])) { s_v[tid] = v; s_i[tid] = i; s_who[tid] = s_who[tid + o]; }
            }
            __syncthreads();
        }
        if (tid == 0) { sel_s[r] = s_v[0]; sel_i[r] = s_v[0] > -INFINITY ? s_i[0] : TS_NONE; }
        if (s_who[0] == tid) ++head;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void trie_beam_expand_kernel(const TrieSearchTable t, const TrieSearchLevel a) {
    __shared__ float s_v[256];
    __shared__ int s_i[256];
    __shared__ int s_who[256];
    __shared__ int s_state[TS_MAXK], s_row[TS_MAXK], s_cnt[TS_MAXK + 1], s_e0[TS_MAXK];
    __shared__ float s_run[TS_MAXK], s_lse[TS_MAXK];
    __shared__ float sel_s[TS_MAXK];
    __shared__ int sel_i[TS_MAXK];
    __shared__ float c_tot[2 * TS_MAXK], c_lp[2 * TS_MAXK], c_stop[2 * TS_MAXK];     // pool candidates: the old pool, then the new
    __shared__ int c_mem[2 * TS_MAXK];
    const int p = blockIdx.x, tid = threadIdx.x, K = a.K, top = a.top;
    const float *__restrict__ logits = a.logits;

    // ---- the beams as they stand (a state outside the table counts as dead)
    if (tid < TS_MAXK) {
        int st = 0;
        float run = -INFINITY;
        if (tid < K && a.flags[3 * p]) {
            st = a.state_in[p * K + tid];
            run = a.score_in[p * K + tid];
            if (st <= 0 || st >= t.n_states || !(run > -INFINITY)) { st = 0; run = -INFINITY; }
        }
        const int row = a.rows_per_prompt == 1 ? p : p * K + tid;
        s_state[tid] = st;
        s_run[tid] = run;
        s_row[tid] = row;
        s_lse[tid] = st ? a.lse[row] : 0.f;
        s_e0[tid] = st ? t.edge_off[st] : 0;
        s_who[tid] = st ? t.edge_off[st + 1] - t.edge_off[st] : 0;                   // (edge count, for the prefix sum below)
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < TS_MAXK; ++k) { s_cnt[k] = acc; acc += s_who[k]; }
        s_cnt[TS_MAXK] = acc;
    }
    // ---- pool candidates: the old pool first
    if (tid < TS_MAXK) {
        const bool have = tid < top && a.pool_member[p * top + tid] >= 0;
        c_mem[tid] = have ? a.pool_member[p * top + tid] : TS_NONE;
        c_lp[tid] = have ? a.pool_lp[p * top + tid] : -INFINITY;
        c_stop[tid] = have ? a.pool_stop[p * top + tid] : 0.f;
        c_tot[tid] = have ? c_lp[tid] + c_stop[tid] : -INFINITY;
        c_mem[TS_MAXK + tid] = TS_NONE;
        c_lp[TS_MAXK + tid] = -INFINITY;
        c_stop[TS_MAXK + tid] = 0.f;
        c_tot[TS_MAXK + tid] = -INFINITY;
    }
    __syncthreads();

    float bs[TS_MAXK];
    int bi[TS_MAXK];
    if (a.include_stop) {
        // a live beam on a member state: its stop term from its own logits (list order), offered with the beam's score
        if (tid < TS_MAXK) {
            const int st = s_state[tid];
            const int m = st ? t.member[st] : -1;
            float stop = -INFINITY;
            if (m >= 0) {
                const float *row = logits + (int64_t)s_row[tid] * a.ld;
                const int set = t.stop_set[st];
                float sum = 0.f;
                for (int j = t.stop_off[set]; j < t.stop_off[set + 1]; ++j) sum += __expf(row[t.stop_ids[j]] - s_lse[tid]);
                stop = __logf(sum);
                const float tot = s_run[tid] + stop;
                if (tot > -INFINITY) { c_mem[TS_MAXK + tid] = m; c_lp[TS_MAXK + tid] = s_run[tid]; c_stop[TS_MAXK + tid] = stop; c_tot[TS_MAXK + tid] = tot; }
            }
            if (a.beam_stop && tid < K) a.beam_stop[p * K + tid] = stop;
        }
    } else {
        // every child that completes a member, keyed by the member index
#pragma unroll
        for (int j = 0; j < TS_MAXK; ++j) { bs[j] = -INFINITY; bi[j] = TS_NONE; }
        for (int k = 0; k < K; ++k) {
            if (!s_state[k]) continue;
            const float *row = logits + (int64_t)s_row[k] * a.ld;
            const float off = s_lse[k], add = s_run[k];
            const int n = s_cnt[k + 1] - s_cnt[k], e0 = s_e0[k];
            for (int e = tid; e < n; e += 256) {
                const int m = t.member[t.edge_next[e0 + e]];
                if (m >= 0) ts_insert(bs, bi, (row[t.edge_tok[e0 + e]] - off) + add, m);
            }
        }
        ts_select(bs, bi, top, s_v, s_i, s_who, sel_s, sel_i);
        if (tid < top && sel_i[tid] != TS_NONE) { c_mem[TS_MAXK + tid] = sel_i[tid]; c_lp[TS_MAXK + tid] = sel_s[tid]; c_tot[TS_MAXK + tid] = sel_s[tid]; }
        if (a.beam_stop && tid < K) a.beam_stop[p * K + tid] = -INFINITY;
    }
    __syncthreads();
    // ---- the pool: `top` rounds over the (at most 32) candidates, one thread
    if (tid == 0) {
        for (int r = 0; r < top; ++r) {
            int best = -1;
            for (int j = 0; j < 2 * TS_MAXK; ++j) {
                if (c_mem[j] == TS_NONE) continue;
                if (best < 0 || c_tot[j] > c_tot[best] || (c_tot[j] == c_tot[best] && c_mem[j] < c_mem[best])) best = j;
            }
            a.pool_member[p * top + r] = best < 0 ? -1 : c_mem[best];
            a.pool_lp[p * top + r] = best < 0 ? -INFINITY : c_lp[best];
            a.pool_stop[p * top + r] = best < 0 ? -INFINITY : c_stop[best];
            if (r == top - 1) s_v[0] = best < 0 ? -INFINITY : c_tot[best];           // the top-th entry: what a live beam has to reach
            if (best >= 0) c_mem[best] = TS_NONE;
        }
    }
    __syncthreads();
    const float need = s_v[0];
    __syncthreads();

    // ---- the K best continuations, keyed by (beam, edge) = the edge's ordinal among the live beams' edges
#pragma unroll
    for (int j = 0; j < TS_MAXK; ++j) { bs[j] = -INFINITY; bi[j] = TS_NONE; }
    int mine = 0;                                        // competitors this thread saw
    for (int k = 0; k < K; ++k) {
        if (!s_state[k]) continue;
        const float *row = logits + (int64_t)s_row[k] * a.ld;
        const float off = s_lse[k], add = s_run[k];
        const int n = s_cnt[k + 1] - s_cnt[k], e0 = s_e0[k], c0 = s_cnt[k];
        for (int e = tid; e < n; e += 256) {
            const int nx = t.edge_next[e0 + e];
            if (!a.include_stop && t.edge_off[nx + 1] == t.edge_off[nx]) continue;    // a leaf is never evaluated
            ++mine;
            ts_insert(bs, bi, (row[t.edge_tok[e0 + e]] - off) + add, c0 + e);
        }
    }
    ts_select(bs, bi, K, s_v, s_i, s_who, sel_s, sel_i);
    s_i[tid] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_i[tid] += s_i[tid + o];
        __syncthreads();
    }
    const int competitors = s_i[0];
    const float best_live = sel_s[0];
    const bool live = best_live > -INFINITY && !(best_live < need);
    if (tid < K) {
        const int ord = live ? sel_i[tid] : TS_NONE;
        int tok = 0, par = p * K + tid, nx = 0;
        float sc = -INFINITY, elp = -INFINITY;
        if (ord != TS_NONE) {
            int k = 0;
            for (int j = 1; j < TS_MAXK; ++j) k = ord >= s_cnt[j] ? j : k;          // the last beam that starts at or before it owns it
            const int e = s_e0[k] + (ord - s_cnt[k]);
            tok = t.edge_tok[e];
            nx = t.edge_next[e];
            par = p * K + k;
            elp = logits[(int64_t)s_row[k] * a.ld + tok] - s_lse[k];
            sc = sel_s[tid];
        }
        a.tok[p * K + tid] = tok;
        a.parent[p * K + tid] = par;
        a.state_out[p * K + tid] = nx;
        a.score_out[p * K + tid] = sc;
        if (a.edge_lp) a.edge_lp[p * K + tid] = elp;
        s_who[tid] = par != p * K + tid;
    }
    __syncthreads();
    if (tid == 0) {
        int moved = 0;
        for (int k = 0; k < K; ++k) moved |= s_who[k];
        a.flags[3 * p] = live ? 1 : 0;
        if (competitors > K) a.flags[3 * p + 1] = 0;                                 // a candidate went without a slot
        a.flags[3 * p + 2] = moved;
    }
}

// words[0] = prompts still live, words[1] = prompts whose beams change rows (0: the level's permutation is the identity)
__global__ __launch_bounds__(64) void trie_search_summary_kernel(const int32_t *__restrict__ flags, int P, int32_t *__restrict__ words) {
    __shared__ int s_a[64], s_b[64];
    int live = 0, moved = 0;
    for (int p = threadIdx.x; p < P; p += 64) { live += flags[3 * p] != 0; moved += flags[3 * p + 2] != 0; }
    s_a[threadIdx.x] = live;
    s_b[threadIdx.x] = moved;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_a[threadIdx.x] += s_a[threadIdx.x + o]; s_b[threadIdx.x] += s_b[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { words[0] = s_a[0]; words[1] = s_b[0]; }
}

hipError_t launch_trie_beam_expand(const TrieSearchTable &t, const TrieSearchLevel &a, int P, int32_t *words, hipStream_t s) {
    if (P < 1 || a.K < 1 || a.K > TS_MAXK || a.top < 1 || a.top > a.K || (a.rows_per_prompt != 1 && a.rows_per_prompt != a.K))
        return hipErrorInvalidValue;
    if (!t.edge_off || !t.member || !t.stop_set || !t.stop_off || !t.stop_ids || t.n_states < 1 || (int64_t)t.n_edges * TS_MAXK >= 0x7fffffff)
        return hipErrorInvalidValue;
    if (!a.logits || !a.lse || !a.state_in || !a.score_in || !a.tok || !a.parent || !a.state_out || !a.score_out || !a.pool_member ||
        !a.pool_lp || !a.pool_stop || !a.flags || !words)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(trie_beam_expand_kernel, dim3(P), dim3(256), 0, s, t, a);
    hipLaunchKernelGGL(trie_search_summary_kernel, dim3(1), dim3(64), 0, s, a.flags, P, words);
    return hipGetLastError();
}

}  // namespace opus
