// Constrained decoding (generate(prefix_allowed_tokens_fn=TokenTrie), transformers' PrefixConstrainedLogitsProcessor): every
// logit outside the set the row's automaton state allows becomes -inf, in place, behind the other logits processors and before
// the arg-max or the sampling head reads the row.
//
// The automaton (opus_set_token_constraint) is a deterministic table in CSR form: state s allows edge_tok[edge_off[s] ..
// edge_off[s + 1]) (ascending; edge_next holds the targets) and, when completing[s] is set, the end ids.  State 0 is the end
// state: no edges, completing - a row that emitted an end id, or an id that was not allowed (a finished row's pads), stays
// there and may only emit end ids.
//
// P workgroups per row (grid B x P, P = 256 / B clamped to 1 .. 8: one workgroup per row stores its 513 KB from one CU, and 64
// rows then use a quarter of the chip - measured 22 us per step at batch 64 against 8 us for the bytes), each owning a slice of
// the vocabulary that starts on a multiple of 32 ids:
//   1. state   thread 0 takes ONE transition from the row's stored state on the id generated last, hist[b * ld + t - 1]
//              (t = *step, the device step word: a captured step serves every call) by binary search in the state's ascending
//              ids, or the row's start state at t == 0.  The history is never walked: the cost of a step does not depend on t.
//              Every slice takes the same transition; the state words are double-buffered by the parity of t (read t - 1's,
//              write t's, slice 0 only), so no slice can read a word another slice of this launch has written.
//   2. set     a bit map of the slice in LDS (at most 19 KB: V = 152 064 in one slice), cleared, then filled from the state's
//              edge list with coalesced reads (the root of a 50 000-member trie has thousands of children) and LDS atomic ORs,
//              plus the end ids.
//   3. mask    one sweep over the slice that STORES -inf where the bit is clear and touches nothing else: the logits are not
//              read, allowed entries keep their bits (penalties applied before included).  16-byte stores where four
//              neighbours are all outside the set (the common case), single stores around an allowed id.
// logits == nullptr advances the state only (opus_debug_token_constraint replays a history one launch per id with it).
#include "common.h"

namespace opus {

constexpr int TC_THREADS = 1024;

__global__ __launch_bounds__(TC_THREADS) void token_constraint_kernel(float *__restrict__ logits, int V, int chunk,
                                                                      const int32_t *__restrict__ hist, int64_t ld,
                                                                      const int32_t *__restrict__ step, int max_hist,
                                                                      const TokenConstraintDesc *__restrict__ dp) {
    extern __shared__ uint32_t s_map[];               // the slice's bits: chunk / 32 words + 1
    __shared__ int32_t s_state;
    const int b = blockIdx.x, tid = threadIdx.x;
    const TokenConstraintDesc d = *dp;
    if (tid == 0) {
        int t = *step;
        t = t < 0 ? 0 : (t > max_hist ? max_hist : t);
        int s;
        if (t == 0) {
            s = d.start[d.n_start > 1 ? b / d.start_div : 0];
        } else {
            int cur = d.state[((t - 1) & 1) * d.state_stride + b];
            if ((unsigned)cur >= (unsigned)d.n_states) cur = 0;
            const int tok = hist[(int64_t)b * ld + t - 1];
            int lo = d.edge_off[cur], hi = d.edge_off[cur + 1];
            while (lo < hi) {                         // first edge whose id is >= tok
                const int mid = (lo + hi) >> 1;
                if (d.edge_tok[mid] < tok) lo = mid + 1; else hi = mid;
            }
            s = (lo < d.edge_off[cur + 1] && d.edge_tok[lo] == tok) ? d.edge_next[lo] : 0;
        }
        if ((unsigned)s >= (unsigned)d.n_states) s = 0;
        if (blockIdx.y == 0) d.state[(t & 1) * d.state_stride + b] = s;
        s_state = s;
    }
    if (!logits) return;
    const int lo = blockIdx.y * chunk, hi = min(V, lo + chunk);        // this slice's ids; lo is a multiple of 32
    if (lo >= hi) return;
    const int wbase = lo >> 5, nw = ((hi - 1) >> 5) - wbase + 1;
    for (int w = tid; w <= nw; w += TC_THREADS) s_map[w] = 0u;         // (one word past the map: the straddle read below)
    __syncthreads();
    const int s = s_state;
    const int e0 = d.edge_off[s], e1 = d.edge_off[s + 1];
    for (int e = e0 + tid; e < e1; e += TC_THREADS) {
        const int id = d.edge_tok[e];
        if (id >= lo && id < hi) atomicOr(&s_map[(id >> 5) - wbase], 1u << (id & 31));
    }
    if (d.completing[s])
        for (int k = tid; k < d.n_end; k += TC_THREADS) {
            const int id = d.end_ids[k];
            if (id >= lo && id < hi) atomicOr(&s_map[(id >> 5) - wbase], 1u << (id & 31));
        }
    __syncthreads();

    float *row = logits + (int64_t)b * V;
    const float ninf = -INFINITY;
    // 16-byte stores need 16-byte aligned addresses: up to 3 single entries, groups of four from i0 on, a tail
    const int r0 = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);   // aligned ids are = r0 (mod 4)
    const int i0 = min(hi, lo + ((r0 - lo) & 3));
    const int n4 = (hi - i0) >> 2;
    if (tid < i0 - lo) {
        const int i = lo + tid;
        if (!((s_map[(i >> 5) - wbase] >> (i & 31)) & 1u)) row[i] = ninf;
    }
    for (int q = tid; q < n4; q += TC_THREADS) {
        const int i = i0 + 4 * q;                     // bits of i .. i + 3 (they may straddle two words)
        const int w = (i >> 5) - wbase, sh = i & 31;
        uint32_t bits = s_map[w] >> sh;
        if (sh > 28) bits |= s_map[w + 1] << (32 - sh);
        bits &= 0xfu;
        if (bits == 0u) {
            *reinterpret_cast<float4 *>(row + i) = make_float4(ninf, ninf, ninf, ninf);
        } else if (bits != 0xfu) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!((bits >> k) & 1u)) row[i + k] = ninf;
        }
    }
    const int t0 = i0 + 4 * n4;
    if (tid < hi - t0) {
        const int i = t0 + tid;
        if (!((s_map[(i >> 5) - wbase] >> (i & 31)) & 1u)) row[i] = ninf;
    }
}

hipError_t launch_token_constraint(float *logits, int B, int V, const int32_t *hist, int64_t ld, const int32_t *step, int max_hist,
                                   const TokenConstraintDesc *desc, hipStream_t s) {
    if (V < 1 || V > TC_MAX_VOCAB || B < 1) return hipErrorInvalidValue;
    int P = logits ? 256 / B : 1;
    P = P < 1 ? 1 : (P > 8 ? 8 : P);
    const int chunk = ((V + P - 1) / P + 31) & ~31;                     // ids per slice, a multiple of 32
    const size_t lds = logits ? (size_t)(chunk / 32 + 1) * sizeof(uint32_t) : 0;
    hipLaunchKernelGGL(token_constraint_kernel, dim3(B, P), dim3(TC_THREADS), lds, s, logits, V, chunk, hist, ld, step, max_hist, desc);
    return hipGetLastError();
}

}  // namespace opus
