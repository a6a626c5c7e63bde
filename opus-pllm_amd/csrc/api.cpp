// C ABI + runtime of libopus_pllm.so: context, weight registry, workspace / KV cache, the kernel
// sequences of the path (encoder, projectors, splice, prefill, decode), the on-device greedy loop
// with hipGraph replay of the decode step, and per-kernel-class event timing for bench.py.
#include "../../include/opus_pllm.h"
#include "common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <vector>

using namespace opus;

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIPC(expr)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(OPUS_EHIP, "%s failed: %s (%s:%d)", #expr,                 \
                                          hipGetErrorString(e_), __FILE__, __LINE__);                \
    } while (0)
#define OPC(expr)                  \
    do {                           \
        int r_ = (expr);           \
        if (r_ != OPUS_OK) return r_; \
    } while (0)

struct Tensor {
    const void *p = nullptr;
    int dtype = -1;
    std::vector<int64_t> shape;
};

struct EncLayer {   // the LayerNorm weights are folded into wqkv / w1 and the biases bqkv / b1 at load time (weights.py);
    const float *bqkv, *bo, *b1, *b2, *sqkv, *s1;   // sqkv / s1: column sums of the folded weights (fused LayerNorm, GemmParams::ln_*)
    const half_t *wqkv, *wo, *w1, *w2;
};
struct DecLayer {   // arch 0: RMSNorm weights are folded into wqkv / wgu (and dec.lnf into lm_head) at load time
    const half_t *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr;
    const float *bqkv = nullptr;                      // Qwen2 q/k/v bias, OPT bias
    // optional quantised form of the four projections (WQ_FORMATS: dec.{l}.{wqkv,wo,wgu,wd}.q8 / .e8 or .q4 / .s4 - the same
    // values as the fp16 tensors, which then hold the dequantised weights); empty: not bound.  Read by the decode step's GEMMs
    // only (GemmAsk::quant).
    QuantW wq_qkv, wq_o, wq_gu, wq_d;
    // arch 1 (OPT / Galactica): LayerNorm affine parameters, fc1 / fc2 and the remaining biases
    const half_t *w1 = nullptr, *w2 = nullptr;
    const float *bo = nullptr, *b1 = nullptr, *b2 = nullptr, *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr;
};

struct TimeRec {
    int klass, phase;
    hipEvent_t e0, e1;
    double bytes, flops;
};

// What decides which launches the head of a decode step makes (select_next) and with which scalar arguments: built once per call
// (generate_impl) or session (opus_stream_begin), the settings of the setter entry points copied in.  What the launches read through
// device descriptors and words (output addresses, processor values, constraint table, guidance scale, T0) is not part of it.
struct StepPlan {
    int rows = -1;                       // decoder rows
    bool guided = false;                 // the rows are guided pairs: the head works on the first rows / 2 (the scale: the word d_gscale)
    int stride = -1;                     // of the id matrix: the token budget (a session: the context's max_new_tokens)
    int32_t *ids = nullptr;              // id buffer [head rows, stride]
    int n_eos = -1, pad = 0;
    float temp = 0.f, top_p = 1.f;       // temp 0: greedy
    int top_k = 0, n_stop = 0;           // opus_set_sampling_top_k, opus_set_stop_sequence
    int outs = 0;                        // GEN_* flags of opus_generate_scored (the addresses come from the descriptors)
    bool lproc = false;                  // logits processors on (their values come from the descriptor d_lproc)
    bool cons = false;                   // token constraint on (its table comes from the descriptor d_cons)
    bool warp = false;                   // sampling warpers on (their values come from the descriptor d_warp)
    int budget = -1;                     // a session's token budget per row (the finish launch); -1: not a session
};
// "the same captured step": the key of the graph cache and of the session's slot
static bool same_step(const StepPlan &a, const StepPlan &b) {
    return a.rows == b.rows && a.guided == b.guided && a.stride == b.stride && a.ids == b.ids && a.n_eos == b.n_eos && a.pad == b.pad &&
           a.temp == b.temp && a.top_p == b.top_p && a.top_k == b.top_k && a.n_stop == b.n_stop && a.outs == b.outs &&
           a.lproc == b.lproc && a.cons == b.cons && a.warp == b.warp && a.budget == b.budget;
}

struct opus_ctx {
    opus_config cfg;
    int device = 0;
    std::map<std::string, Tensor> w;
    bool resolved = false;
    // resolved weights
    const half_t *enc_emb = nullptr, *dec_emb = nullptr, *lm_head = nullptr, *proj_w = nullptr, *dec_pos = nullptr;
    const float *enc_lnfw = nullptr, *enc_lnfb = nullptr, *proj_b = nullptr, *dec_lnfw = nullptr, *dec_lnfb = nullptr;
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;
    std::vector<const half_t *> sw_w;
    std::vector<const float *> sw_b;
    // workspace
    char *ws = nullptr;
    size_t ws_bytes = 0;
    float *e_x, *e_hid, *p_pool_dummy, *e_part, *e_stat;
    int32_t *e_cu, *e_pos;
    std::vector<int32_t> h_cu;           // host copy of the packed encoder's row offsets (source of the async upload)
    int64_t enc_rows = 0;                // token rows of e_hid the last encoder call left complete (0: none - opus_esm2_lm_head refuses)
    half_t *e_xn, *e_qkv, *e_ctx, *e_h1;
    half_t *p_xn, *p_y, *p_z[2];
    float *d_x, *d_xl, *d_logits, *d_pval, *gemm_ws, *d_probs, *d_zpart, *d_spart, *d_part, *d_stat;
    int32_t *d_cand_i, *d_cand_n;
    uint64_t *d_seed;
    int32_t *d_chosen;
    int samp_top_k = 0;                       // opus_set_sampling_top_k (0 = no TopKLogitsWarper)
    float *d_bthr = nullptr, *d_blse = nullptr;   // beam-sample: keep threshold and log-sum-exp per decoder row
    // sampling warpers (opus_set_sampling_warpers): the host setting, uploaded in stream order by every call that samples with one
    // on, and a small allocation made on first use - the device descriptor and the band's bounds per row [2, max_batch]
    SamplingWarpers h_warp{0.f, 1.f, 0.f, 0.f};
    char *warp_mem = nullptr;
    SamplingWarpers *d_warp = nullptr;
    float *d_wlo = nullptr, *d_whi = nullptr;
    bool warp_on() const { return h_warp.min_p > 0.f || h_warp.typical_p < 1.f || h_warp.epsilon > 0.f || h_warp.eta > 0.f; }
    int64_t gemm_ws_bytes = 0;
    half_t *d_xn, *d_qkv, *d_ctx, *d_act, *d_xln, *kc, *vc;
    float *cs_enc, *cs_dec, *cs_row;
    int32_t *d_kstart, *d_step, *d_next, *d_fin, *d_nunf, *d_eos, *d_plan, *d_pidx, *d_stop, *d_cnt;
    int n_stop = 0;                      // opt-in stop sequence (opus_set_stop_sequence)
    // "has every row finished?" is polled with a bounded run-ahead (generate_impl): the step's unfinished count lands in pinned host
    // memory behind an event per step
    static constexpr int POLL_RING = 4, POLL_LAG = 2;
    int32_t *h_nunf = nullptr;
    hipEvent_t poll_ev[POLL_RING] = {nullptr, nullptr, nullptr, nullptr};
    int64_t cache_sl, cache_sb, cache_sh;   // strides (halfs): layer, batch row, kv head
    // decode state
    int cur_B = 0, cur_T = 0;
    bool prefilled = false;
    // Graph cache for the decode iteration.  A captured step does NOT depend on the prompt length: T0 reaches its kernels through
    // the device word d_step[1] (d_step[0] = the step counter), so one instantiated graph serves every batch of a dataset whatever
    // its T.  It does depend on everything in the step's plan (the number of rows: grid sizes, kernel routing; the token budget:
    // stride of the id matrix; the pad / EOS / sampling settings, the id buffer, the mode of the head): a few entries are kept (a
    // dataset's full batches + its short last batch), least recently used first out.
    struct GraphEntry {
        hipGraphExec_t exec = nullptr;
        StepPlan key;
        uint64_t used = 0;
    };
    static constexpr int MAX_GRAPHS = 4;
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int64_t graph_instantiations = 0;    // opus_stat("graph_instantiations")
    int64_t graph_replays = 0;
    int64_t decode_steps = 0;            // decode steps enqueued by opus_generate_* (eager or from a graph)
    // opus_generate_scored's outputs: a separate small allocation (first use), not the workspace - the descriptor of the call's
    // output addresses (h_gen, copied to d_gen before the loop), the part sums of the fused log-sum-exp and the draw's thresholds
    char *gen_mem = nullptr;
    GenOutDesc *d_gen = nullptr;
    GenOutDesc h_gen{};
    float *d_gpsum = nullptr, *d_gthr = nullptr;
    // top log-probs (opus_set_gen_top_logprobs; 0: off): the caller's buffers, and an allocation made on first use - the parts'
    // candidate keys [topk_rows(), APART, TOPK_MAX] and (opus_debug_top_logprobs) the rows' log-sum-exp
    int top_k = 0;
    int32_t *top_ids = nullptr;
    float *top_lp = nullptr;
    char *topk_mem = nullptr;
    uint64_t *d_tcand = nullptr;
    float *d_tlse = nullptr;
    float *fwd_lse = nullptr;            // opus_llama_forward with top log-probs on: a chunk's log-sum-exp rows (grown on use)
    int64_t fwd_lse_cap = 0;
    int topk_rows() const { return cfg.max_batch > 64 ? cfg.max_batch : 64; }
    // logits processors (opus_set_logits_processors): the host setting, uploaded in stream order by every generate call, and a
    // separate allocation made on first use - the device descriptor, the step word of opus_debug_logits_process, the output
    // descriptors split into raw (before the processors) and processed (after), the raw rows' log-sum-exp and the raw logits of the
    // history positions [max_batch, max_new_tokens]
    bool lproc_on = false;
    LogitsProcDesc h_lproc{1.0f, 0, 0, 0, {}, {}};
    char *lproc_mem = nullptr;
    LogitsProcDesc *d_lproc = nullptr;
    int32_t *d_lstep = nullptr, *d_ridx = nullptr;
    GenOutDesc *d_gen_raw = nullptr, *d_gen_proc = nullptr;
    float *d_rlse = nullptr, *d_rawh = nullptr;
    // token constraint (opus_set_token_constraint): the automaton's table in an allocation of its own, grown on use (cons_tab), and
    // a small fixed one made on first use (cons_mem) - the device descriptor the captured step reads, the rows' state words
    // [2, max_batch] (double-buffered by the step's parity) and the step word of opus_debug_token_constraint
    bool cons_on = false;
    char *cons_tab = nullptr, *cons_mem = nullptr;
    size_t cons_tab_bytes = 0;
    TokenConstraintDesc *d_cons = nullptr;
    int32_t *d_cstate = nullptr, *d_cstep = nullptr;
    int32_t cons_n_start = 0, cons_max_id = -1;
    int32_t cons_start_div = 1;          // TokenConstraintDesc::start_div as the device descriptor holds it
    // classifier-free guidance (opus_generate_scored_guided; StepPlan::guided): rows [0, cur_B / 2) are the conditional prompts the
    // head of the step works on and rows [cur_B / 2, cur_B) their negative prompts.  guid_mem (first use): the scale word the
    // captured step reads, the part sums and the rows' maximum / log of the shifted sum / log-sum-exp [2 max_batch each]; guid_keep (first
    // guided call with token log-probs): the raw conditional rows [max_batch / 2, V] the combine overwrites in d_logits
    char *guid_mem = nullptr;
    float *d_gscale = nullptr, *d_gdpsum = nullptr, *d_gmax = nullptr, *d_glog = nullptr, *d_glse = nullptr, *guid_keep = nullptr;
    int gemm_wq = WQ_NONE;               // the quantised format this context's last GEMM streamed (GemmParams::ran_wq)
    int64_t wq_gemms[WQ_COUNT] = {};     // GEMMs issued on this context per streamed format (opus_stat("w8_gemms"), "w4_gemms")
    int gemm_plan[GEMM_PLAN_WORDS] = {-1, -1, -1, -1, -1, -1, -1, -1};   // the launchers' report of this context's last GEMM (GemmParams::plan; opus_debug_gemm_plan)
    // row-scale fusion (GemmParams::ssq_out / row_ssq): the rows' sums of squares, written by the GEMM that is asked for the fp16
    // copy of its output (GemmAsk::xh) and read by the one that scales its rows (GemmAsk::rs_on)
    float *d_ssq = nullptr;
    int64_t ssq_cap = 0;                 // floats in d_ssq
    // timing
    bool timing = false;
    int phase = PH_OTHER;
    std::vector<TimeRec> recs;
    // rows the projector workspace (p_xn, p_y, p_z) holds: larger batches are projected in chunks of this many rows.  The
    // context's own workspace holds max_batch rows; the first call with more rows (the batched stage of the two-stage
    // pipeline) allocates a separate BIG_PROJ_ROWS-row workspace (proj_big) and switches to it.
    int proj_rows = 0;
    char *proj_big = nullptr;
    // beam search (opus_beam_topk / opus_kv_reorder): one layer's K and V cache rows while they are permuted (first use allocates)
    half_t *kv_tmp = nullptr;
    // trie search (opus_set_trie_search): the table in an allocation of its own, grown on use; ts.edge_off == nullptr: none set
    char *ts_tab = nullptr;
    size_t ts_tab_bytes = 0;
    TrieSearchTable ts{};
    int32_t ts_max_id = -1;
    // cache epoch: a new value (process-wide unique, so that a handle of another context never matches) whenever a call prefills or
    // permutes the KV cache; opus_llama_prefix hands it out, opus_llama_score_continuations checks it.  h_kstart: the first real
    // slot of every row of the last opus_llama_prefix (host copy for the continuation rows' positions).
    int64_t epoch = 0;
    std::vector<int32_t> h_kstart;
    // opus_llama_prefill_behind's int32 tables (row lists, positions, lengths, workgroup table, gather index): an allocation of
    // its own, made on first use for the largest pass the context can run
    int32_t *behind_tbl = nullptr;
    int64_t prefills_behind = 0;         // opus_stat("prefills_behind")
    // continuous batching (opus_stream_*): one live decode batch whose done rows are refilled.  stream_mem (first use): start [B],
    // poll [B + 1] (end steps + the count of rows not done), the refill's tables (new kstart per row, listed rows, their snapshot
    // rows, kv_place's offsets and list).  h_poll (pinned): STREAM_RING copies of poll, one per step in flight.  The captured step
    // of a session is an entry of its own (stream_graph), beside the plain graphs and never evicting one.
    static constexpr int STREAM_LAG = POLL_LAG + 1, STREAM_RING = POLL_RING;
    struct StreamState {
        bool on = false;
        int T0 = 0, t = 0;
        StepPlan plan;                   // rows, budget, id buffer [rows, max_new_tokens] ... of the session's step
        std::vector<int32_t> start;      // host copy of start[]
    } st;
    char *stream_mem = nullptr;
    int32_t *d_sstart = nullptr, *d_spoll = nullptr, *d_snks = nullptr, *d_srows = nullptr, *d_ssrc = nullptr, *d_soff = nullptr,
            *d_slist = nullptr;
    int32_t *h_poll = nullptr;
    GraphEntry stream_graph;
    int64_t stream_steps = 0, stream_refills = 0;   // opus_stat("stream_steps" / "stream_refills")
    // prompt-lookup decoding (opus_generate_lookup / opus_llama_verify_step).  lk_mem (first use): the token matrix of a pass
    // [max_batch] (row b: the last committed id, then the draft), the rows' draft lengths, history lengths and arg-maxes
    // [max_batch each], the EOS / stop ids of opus_debug_lookup_accept, the pass's words {a, unfinished, step, drafted, longest draft}.
    // h_lk (pinned): the words the host reads once per pass.  lk_kstart: host copy of kstart of the prefill of epoch lk_epoch.
    char *lk_mem = nullptr;
    int32_t *d_lk_tok = nullptr, *d_lk_dlen = nullptr, *d_lk_hlen = nullptr, *d_lk_arg = nullptr, *d_lk_ids = nullptr, *d_lk_words = nullptr;
    int32_t *h_lk = nullptr;
    std::vector<int32_t> lk_kstart;
    int64_t lk_epoch = -1;
    int64_t lookup_passes = 0;           // opus_stat("lookup_passes")
};

static std::atomic<int64_t> g_epoch{0};
static void new_epoch(opus_ctx *c) {     // (a call that prefills or permutes the cache also ends a continuous session)
    c->epoch = ++g_epoch;
    c->st.on = false;
}

// Continuation rows of opus_llama_score_continuations in the prefill's layer loop: B rows of T new positions behind a cached prefix.
// No mask / kstart upload, no cache write, no decode state: rotary (learned positions for OPT) at Tp - kstart[p] + t through
// nkst[b] = kstart[p] - Tp, and attn_prefix_kernel instead of the causal prefill attention.  opus_llama_score_tree runs trie nodes
// the same way: T = 1, nkst[b] = kstart[p] - Tp - (depth - 1), and attn.par set selects the kernel's tree form.
struct ContRows {
    const int32_t *nkst;          // [B] device
    AttnPrefixParams attn;        // layer-independent fields (kc / vc are set per layer)
    int nblocks;
    // a detached prefix (opus_prefix_snap): the layers' K / V come from the snapshot (layer stride snap_sl halfs; attn.cache_sb /
    // cache_sh / kstart are the snapshot's) instead of the context's cache
    const half_t *snap_k = nullptr, *snap_v = nullptr;
    int64_t snap_sl = 0;
    // opus_llama_prefill_behind: the rows' rotated K and V of positions t < app_lens[b] (device, [B]) are also appended to cache
    // row b at slot attn.Tp + (T - app_lens[b]) + t
    const int32_t *app_lens = nullptr;
    // a verify pass of prompt-lookup decoding: the per-layer GEMMs ask for the FP8 panels as the decode step does, phase "decode"
    bool w8 = false;
};

// ------------------------------------------------------------------------------------------------
static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carver {
    char *base;
    size_t off = 0;
    template <class T>
    T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += align_up(n * sizeof(T));
        return p;
    }
};

static void carve(opus_ctx *c, char *base, size_t *total) {
    const opus_config &g = c->cfg;
    Carver k{base};
    const size_t Me = (size_t)g.max_batch * g.max_enc_tokens;
    const size_t De = g.enc_dim, Fe = g.enc_ffn;
    c->e_x = k.take<float>(Me * De);
    c->e_hid = k.take<float>(Me * De);
    c->e_xn = k.take<half_t>(Me * De);
    c->e_qkv = k.take<half_t>(Me * 3 * De);
    c->e_ctx = k.take<half_t>(Me * De);
    c->e_h1 = k.take<half_t>(Me * Fe);
    c->e_part = k.take<float>(Me * (De / 64 + 1) * 2);              // (sum x, sum x^2) per row and 64-column slab (fused LayerNorm)
    c->e_stat = k.take<float>(Me * 2);                              // (mu, rstd) per row
    c->e_cu = k.take<int32_t>((size_t)g.max_batch + 4);            // token-packed encoder: row offsets, row -> position table
    c->e_pos = k.take<int32_t>(Me);
    const size_t B = g.max_batch, H = g.dec_dim, SW = (size_t)g.dec_dim * g.n_prot_tokens;
    const size_t PR = B;                         // (the two-stage pipeline's big workspace is allocated on first use: ensure_proj_rows)
    c->proj_rows = (int)PR;
    c->p_xn = k.take<half_t>(PR * De);
    c->p_y = k.take<half_t>(PR * (size_t)(g.has_protein_projector ? g.proj_dim : g.enc_dim));
    c->p_z[0] = k.take<half_t>(PR * SW);
    c->p_z[1] = k.take<half_t>(PR * SW);
    // rows of the decoder activation buffers: whole 16-row tiles, so that the fragment-ordered layout of the batched decode
    // step (tiled_off) fits for every batch size
    const size_t B16 = (B + 15) & ~(size_t)15;
    const size_t Md = B * g.max_prompt > B16 ? B * g.max_prompt : B16;
    const size_t QKV = (size_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim;
    const size_t QD = (size_t)g.dec_heads * g.dec_head_dim;
    c->d_x = k.take<float>(Md * H);
    c->d_xn = k.take<half_t>(Md * H);
    c->d_qkv = k.take<half_t>(Md * QKV);
    c->d_ctx = k.take<half_t>(Md * QD);
    c->d_act = k.take<half_t>(Md * g.dec_ffn);
    c->d_part = k.take<float>(Md * (H / 64 + 1) * 2);               // prefill RMSNorm fused around the big GEMM: partials, (0, rstd)
    c->d_stat = k.take<float>(Md * 2);
    c->d_xl = k.take<float>(B * H);
    c->d_xln = k.take<half_t>(B16 * H);
    c->d_logits = k.take<float>(B * (size_t)g.dec_vocab);
    const size_t ctx = (size_t)g.max_prompt + g.max_new_tokens;
    c->cache_sh = (int64_t)ctx * g.dec_head_dim;
    c->cache_sb = c->cache_sh * g.dec_kv_heads;
    c->cache_sl = c->cache_sb * g.max_batch;
    c->kc = k.take<half_t>((size_t)c->cache_sl * g.dec_layers);
    c->vc = k.take<half_t>((size_t)c->cache_sl * g.dec_layers);
    const size_t maxpos_e = g.max_enc_tokens, maxpos_d = ctx;
    c->cs_enc = k.take<float>(maxpos_e * (g.enc_dim / g.enc_heads));
    c->cs_dec = k.take<float>(maxpos_d * g.dec_head_dim);
    c->cs_row = k.take<float>(B * (size_t)g.dec_head_dim);          // (cos, sin) rows of the current decode step, one per batch row
    c->d_kstart = k.take<int32_t>(B + 4);
    c->d_step = k.take<int32_t>(4);
    c->d_next = k.take<int32_t>(B);
    c->d_fin = k.take<int32_t>(B);
    c->d_nunf = k.take<int32_t>((size_t)g.max_new_tokens + 4);
    c->d_eos = k.take<int32_t>(64);
    c->d_stop = k.take<int32_t>(16);
    c->d_cnt = k.take<int32_t>(HANDOFF_WORDS);                      // ticket / flag words of the in-launch hand-offs + the error word (GemmParams::combine_cnt)
    c->d_plan = k.take<int32_t>(4 * B + 8);
    c->d_pval = k.take<float>(64 * B);
    c->d_probs = k.take<float>(B * ((size_t)g.dec_vocab + 64 * 4));     // candidate probabilities (per-part slots)
    c->d_cand_i = k.take<int32_t>(B * ((size_t)g.dec_vocab + 64 * 4));
    c->d_cand_n = k.take<int32_t>(64 * B);
    c->d_zpart = k.take<float>(64 * B);
    c->d_bthr = k.take<float>(B);
    c->d_blse = k.take<float>(B);
    c->d_spart = k.take<float>(64 * B);
    c->d_seed = k.take<uint64_t>(2);
    c->d_chosen = k.take<int32_t>(B);
    c->gemm_ws_bytes = 64ll << 20;   // split-K slabs of the tile GEMM
    c->gemm_ws = k.take<float>((size_t)c->gemm_ws_bytes / sizeof(float));
    c->d_pidx = k.take<int32_t>(64 * B);
    // per-row sums of squares of the row-scale RMSNorm fusion: up to 128 rows x one float per 16 columns of the residual stream
    c->ssq_cap = 128 * (int64_t)(g.dec_dim / 16 > 32 ? g.dec_dim / 16 : 32);
    c->d_ssq = k.take<float>((size_t)c->ssq_cap);
    *total = k.off;
}

static int check_cfg(const opus_config *g) {
    if (!g) return fail(OPUS_EBADARG, "config is null");
    if (g->enc_layers < 1 || g->dec_layers < 1 || g->enc_heads < 1 || g->dec_heads < 1 || g->dec_kv_heads < 1)
        return fail(OPUS_EBADARG, "layer/head counts must be positive");
    if (g->enc_dim % g->enc_heads) return fail(OPUS_ESHAPE, "enc_dim %% enc_heads != 0");
    const int ehd = g->enc_dim / g->enc_heads;
    auto okhd = [](int h) { return h == 16 || h == 32 || h == 64 || h == 128; };
    if (!okhd(ehd) || !okhd(g->dec_head_dim)) return fail(OPUS_ESHAPE, "head_dim must be 16/32/64/128");
    if (g->dec_heads % g->dec_kv_heads || g->dec_heads / g->dec_kv_heads > 8)
        return fail(OPUS_ESHAPE, "dec_heads / dec_kv_heads must be an integer <= 8");
    const int ks[] = {g->enc_dim, g->enc_ffn, g->dec_dim, g->dec_ffn, g->dec_heads * g->dec_head_dim,
                      g->has_protein_projector ? g->proj_dim : 64, g->dec_dim * g->n_prot_tokens};
    for (int k : ks)
        if (k % 64) return fail(OPUS_ESHAPE, "every GEMM reduction dim must be a multiple of 64 (got %d)", k);
    if (g->enc_dim > 5120 || g->dec_dim > 5120) return fail(OPUS_ESHAPE, "norm width > 5120 unsupported");
    if (g->switch_depth < 1 || g->n_prot_tokens < 1) return fail(OPUS_EBADARG, "switch_depth/n_prot_tokens");
    if (g->max_batch < 1 || g->max_enc_tokens < 3 || g->max_prompt < 1 || g->max_new_tokens < 1)
        return fail(OPUS_EBADARG, "capacity fields must be positive");
    if (g->dec_arch != 0 && g->dec_arch != 1) return fail(OPUS_EBADARG, "dec_arch must be 0 (Llama/Qwen2) or 1 (OPT/Galactica)");
    if (g->dec_arch == 1) {
        if (g->dec_heads != g->dec_kv_heads) return fail(OPUS_ESHAPE, "OPT attention is multi-head: dec_kv_heads == dec_heads");
        if (g->dec_act != 0 && g->dec_act != 1) return fail(OPUS_EUNSUPPORTED, "OPT activation: 0 = GELU (Galactica) or 1 = ReLU (facebook/opt-*)");
        if (g->dec_ffn & 7) return fail(OPUS_ESHAPE, "dec_ffn must be a multiple of 8");
        if (g->max_prompt + g->max_new_tokens > g->dec_max_pos)
            return fail(OPUS_ESHAPE, "max_prompt + max_new_tokens exceeds the learned position table (dec_max_pos=%d)", g->dec_max_pos);
    }
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int opus_abi_version(void) { return OPUS_ABI_VERSION; }
extern "C" int opus_operand_dtype(void) {
#ifdef OPUS_BF16
    return 1;
#else
    return 0;
#endif
}
extern "C" const char *opus_last_error(void) { return g_err; }

extern "C" int64_t opus_workspace_bytes(const opus_config *cfg) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    opus_ctx tmp;
    tmp.cfg = *cfg;
    size_t total = 0;
    carve(&tmp, nullptr, &total);
    return (int64_t)total;
}

static void fill_cs(std::vector<float> &t, int maxpos, int hd, float theta) {
    const int half = hd / 2;
    t.resize((size_t)maxpos * half * 2);
    for (int i = 0; i < half; ++i) {
        // fp32 inv_freq as torch computes it, angle evaluated in double
        const float inv = 1.0f / powf(theta, (float)(2 * i) / (float)hd);
        for (int p = 0; p < maxpos; ++p) {
            const float ang = (float)p * inv;
            t[((size_t)p * half + i) * 2] = (float)cos((double)ang);
            t[((size_t)p * half + i) * 2 + 1] = (float)sin((double)ang);
        }
    }
}

extern "C" int opus_ctx_create(const opus_config *cfg, int device, opus_ctx **out) {
    if (!out) return fail(OPUS_EBADARG, "out is null");
    OPC(check_cfg(cfg));
    HIPC(hipSetDevice(device));
    opus_ctx *c = new opus_ctx();
    c->cfg = *cfg;
    c->device = device;
    size_t total = 0;
    carve(c, nullptr, &total);
    hipError_t e = hipMalloc((void **)&c->ws, total);
    if (e != hipSuccess) {
        delete c;
        return fail(OPUS_EHIP, "hipMalloc(%zu bytes of workspace) failed: %s", total, hipGetErrorString(e));
    }
    c->ws_bytes = total;
    carve(c, c->ws, &total);
    std::vector<float> t;
    fill_cs(t, cfg->max_enc_tokens, cfg->enc_dim / cfg->enc_heads, cfg->enc_rope_theta);
    HIPC(hipMemcpy(c->cs_enc, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    fill_cs(t, cfg->max_prompt + cfg->max_new_tokens, cfg->dec_head_dim, cfg->dec_rope_theta);
    if (cfg->dec_arch == 1)      // no rotary in OPT: (cos, sin) = (1, 0) makes the fused rotate-and-cache kernels plain copies
        for (size_t i = 0; i < t.size(); i += 2) { t[i] = 1.0f; t[i + 1] = 0.0f; }
    HIPC(hipMemcpy(c->cs_dec, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPC(hipMemset(c->d_step, 0, 16));
    HIPC(hipMemset(c->d_cnt, 0, HANDOFF_WORDS * sizeof(int32_t)));
    // the decode attention reads whole 32-slot tiles and masks afterwards: every cache slot must hold finite values
    HIPC(hipMemset(c->kc, 0, (size_t)c->cache_sl * cfg->dec_layers * sizeof(half_t)));
    HIPC(hipMemset(c->vc, 0, (size_t)c->cache_sl * cfg->dec_layers * sizeof(half_t)));
    HIPC(hipHostMalloc((void **)&c->h_nunf, ((size_t)cfg->max_new_tokens + 4) * sizeof(int32_t), hipHostMallocDefault));
    for (auto &e : c->poll_ev) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = c;
    return OPUS_OK;
}

static void timing_clear(opus_ctx *c) {
    for (auto &r : c->recs) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    c->recs.clear();
}

static void drop_graphs(opus_ctx *c) {   // a captured step holds weight pointers, the stop sequence, top-k, knobs ...
    for (auto &g : c->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
    if (c->stream_graph.exec) (void)hipGraphExecDestroy(c->stream_graph.exec);
    c->stream_graph = opus_ctx::GraphEntry();
}

extern "C" int opus_ctx_destroy(opus_ctx *c) {
    if (!c) return OPUS_OK;
    (void)hipSetDevice(c->device);
    timing_clear(c);
    drop_graphs(c);
    if (c->ws) (void)hipFree(c->ws);
    if (c->proj_big) (void)hipFree(c->proj_big);
    if (c->kv_tmp) (void)hipFree(c->kv_tmp);
    if (c->gen_mem) (void)hipFree(c->gen_mem);
    if (c->topk_mem) (void)hipFree(c->topk_mem);
    if (c->fwd_lse) (void)hipFree(c->fwd_lse);
    if (c->lproc_mem) (void)hipFree(c->lproc_mem);
    if (c->warp_mem) (void)hipFree(c->warp_mem);
    if (c->cons_tab) (void)hipFree(c->cons_tab);
    if (c->ts_tab) (void)hipFree(c->ts_tab);
    if (c->cons_mem) (void)hipFree(c->cons_mem);
    if (c->guid_mem) (void)hipFree(c->guid_mem);
    if (c->guid_keep) (void)hipFree(c->guid_keep);
    if (c->behind_tbl) (void)hipFree(c->behind_tbl);
    if (c->h_nunf) (void)hipHostFree(c->h_nunf);
    if (c->stream_mem) (void)hipFree(c->stream_mem);
    if (c->h_poll) (void)hipHostFree(c->h_poll);
    if (c->lk_mem) (void)hipFree(c->lk_mem);
    if (c->h_lk) (void)hipHostFree(c->h_lk);
    for (auto &e : c->poll_ev) if (e) (void)hipEventDestroy(e);
    delete c;
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ weights
// The quantised forms a decoder projection W [N, K] may be bound in: the suffix and dtype of the code tensor [N, K / codes_kdiv]
// and of the scale tensor ([N, K / scales_kdiv]; scales_kdiv 0: one scale per row, [N]).
struct WqFormat {
    int fmt;
    const char *name;
    const char *codes_sfx; int codes_dtype; int64_t codes_kdiv;
    const char *scales_sfx; int scales_dtype; int64_t scales_kdiv;
};
static const WqFormat WQ_FORMATS[] = {
    {WQ_FP8, "FP8", ".q8", OPUS_F8E4M3, 1, ".e8", OPUS_I8, 0},
    {WQ_MXFP4, "MXFP4", ".q4", OPUS_F4E2M1X2, 2, ".s4", OPUS_E8M0, 32},
};

extern "C" int opus_bind_weight(opus_ctx *c, const char *name, const void *d_ptr, int dtype, int ndim,
                                const int64_t *shape) {
    if (!c || !name || !d_ptr || !shape) return fail(OPUS_EBADARG, "null argument");
    if (ndim < 1 || ndim > 4) return fail(OPUS_EBADARG, "ndim %d", ndim);
    const size_t nlen = strlen(name);
    int want = -1;                       // the dtype that the name's suffix asks for (-1: an ordinary weight)
    for (const WqFormat &f : WQ_FORMATS) {
        if (nlen > 3 && !strcmp(name + nlen - 3, f.codes_sfx)) want = f.codes_dtype;
        if (nlen > 3 && !strcmp(name + nlen - 3, f.scales_sfx)) want = f.scales_dtype;
    }
    if (want >= 0 ? dtype != want : (dtype != OPUS_F16 && dtype != OPUS_F32))
        return fail(OPUS_EBADARG, "weights are fp16 or fp32 (FP8 panels '*.q8': e4m3, their row exponents '*.e8': int8; MXFP4 code panels "
                                  "'*.q4': packed e2m1 pairs, their scale panels '*.s4': e8m0)");
    if (((uintptr_t)d_ptr) & 15) return fail(OPUS_EBADARG, "%s: pointer must be 16-byte aligned", name);
    Tensor t;
    t.p = d_ptr;
    t.dtype = dtype;
    t.shape.assign(shape, shape + ndim);
    c->w[name] = t;
    c->resolved = false;
    // a captured decode graph holds the device pointers of the weights it was recorded with
    drop_graphs(c);
    return OPUS_OK;
}

static int getw(opus_ctx *c, const std::string &name, int dtype, std::vector<int64_t> shape, const void **out) {
    auto it = c->w.find(name);
    if (it == c->w.end()) return fail(OPUS_ESTATE, "weight '%s' is not bound", name.c_str());
    const Tensor &t = it->second;
    if (t.dtype != dtype) return fail(OPUS_ESHAPE, "weight '%s' has dtype %d, expected %d", name.c_str(), t.dtype, dtype);
    if (t.shape != shape) {
        std::string got, exp;
        for (auto v : t.shape) got += std::to_string(v) + ",";
        for (auto v : shape) exp += std::to_string(v) + ",";
        return fail(OPUS_ESHAPE, "weight '%s' has shape [%s] expected [%s]", name.c_str(), got.c_str(), exp.c_str());
    }
    *out = t.p;
    return OPUS_OK;
}
#define GW(name, dt, shape, dst) OPC(getw(c, name, dt, shape, reinterpret_cast<const void **>(&(dst))))

extern "C" int opus_weights_ready(opus_ctx *c) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (c->resolved) return OPUS_OK;
    const opus_config &g = c->cfg;
    const int64_t De = g.enc_dim, Fe = g.enc_ffn, H = g.dec_dim, F = g.dec_ffn, V = g.dec_vocab;
    const int64_t QKV = (int64_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim, QD = (int64_t)g.dec_heads * g.dec_head_dim;
    GW("enc.emb", OPUS_F16, (std::vector<int64_t>{g.enc_vocab, De}), c->enc_emb);
    c->enc.resize(g.enc_layers);
    for (int l = 0; l < g.enc_layers; ++l) {
        const std::string p = "enc." + std::to_string(l) + ".";
        EncLayer &L = c->enc[l];
        GW(p + "wqkv", OPUS_F16, (std::vector<int64_t>{3 * De, De}), L.wqkv);
        GW(p + "bqkv", OPUS_F32, (std::vector<int64_t>{3 * De}), L.bqkv);
        GW(p + "sqkv", OPUS_F32, (std::vector<int64_t>{3 * De}), L.sqkv);
        GW(p + "wo", OPUS_F16, (std::vector<int64_t>{De, De}), L.wo);
        GW(p + "bo", OPUS_F32, (std::vector<int64_t>{De}), L.bo);
        GW(p + "w1", OPUS_F16, (std::vector<int64_t>{Fe, De}), L.w1);
        GW(p + "b1", OPUS_F32, (std::vector<int64_t>{Fe}), L.b1);
        GW(p + "s1", OPUS_F32, (std::vector<int64_t>{Fe}), L.s1);
        GW(p + "w2", OPUS_F16, (std::vector<int64_t>{De, Fe}), L.w2);
        GW(p + "b2", OPUS_F32, (std::vector<int64_t>{De}), L.b2);
    }
    GW("enc.lnf.w", OPUS_F32, (std::vector<int64_t>{De}), c->enc_lnfw);
    GW("enc.lnf.b", OPUS_F32, (std::vector<int64_t>{De}), c->enc_lnfb);
    int64_t din = De;
    if (g.has_protein_projector) {
        GW("proj.w", OPUS_F16, (std::vector<int64_t>{g.proj_dim, De}), c->proj_w);
        GW("proj.b", OPUS_F32, (std::vector<int64_t>{g.proj_dim}), c->proj_b);
        din = g.proj_dim;
    }
    const int64_t SW = H * g.n_prot_tokens;
    c->sw_w.resize(g.switch_depth);
    c->sw_b.resize(g.switch_depth);
    for (int i = 0; i < g.switch_depth; ++i) {
        const std::string p = "sw." + std::to_string(i) + ".";
        GW(p + "w", OPUS_F16, (std::vector<int64_t>{SW, din}), c->sw_w[i]);
        GW(p + "b", OPUS_F32, (std::vector<int64_t>{SW}), c->sw_b[i]);
        din = SW;
    }
    GW("dec.emb", OPUS_F16, (std::vector<int64_t>{V, H}), c->dec_emb);
    c->dec.resize(g.dec_layers);
    for (int l = 0; l < g.dec_layers; ++l) {
        const std::string p = "dec." + std::to_string(l) + ".";
        DecLayer &L = c->dec[l];
        GW(p + "wqkv", OPUS_F16, (std::vector<int64_t>{QKV, H}), L.wqkv);
        GW(p + "wo", OPUS_F16, (std::vector<int64_t>{H, QD}), L.wo);
        if (g.dec_arch == 1) {
            GW(p + "ln1.w", OPUS_F32, (std::vector<int64_t>{H}), L.ln1w);
            GW(p + "ln1.b", OPUS_F32, (std::vector<int64_t>{H}), L.ln1b);
            GW(p + "bqkv", OPUS_F32, (std::vector<int64_t>{QKV}), L.bqkv);
            GW(p + "bo", OPUS_F32, (std::vector<int64_t>{H}), L.bo);
            GW(p + "ln2.w", OPUS_F32, (std::vector<int64_t>{H}), L.ln2w);
            GW(p + "ln2.b", OPUS_F32, (std::vector<int64_t>{H}), L.ln2b);
            GW(p + "w1", OPUS_F16, (std::vector<int64_t>{F, H}), L.w1);
            GW(p + "b1", OPUS_F32, (std::vector<int64_t>{F}), L.b1);
            GW(p + "w2", OPUS_F16, (std::vector<int64_t>{H, F}), L.w2);
            GW(p + "b2", OPUS_F32, (std::vector<int64_t>{H}), L.b2);
            continue;
        }
        if (g.dec_qkv_bias) GW(p + "bqkv", OPUS_F32, (std::vector<int64_t>{QKV}), L.bqkv);
        GW(p + "wgu", OPUS_F16, (std::vector<int64_t>{2 * F, H}), L.wgu);
        GW(p + "wd", OPUS_F16, (std::vector<int64_t>{H, F}), L.wd);
        // the optional quantised form, per projection: both tensors of a format or neither, and one format at the most
        const struct { const char *n; int64_t N, K; QuantW *q; } proj[4] = {
            {"wqkv", QKV, H, &L.wq_qkv}, {"wo", H, QD, &L.wq_o}, {"wgu", 2 * F, H, &L.wq_gu}, {"wd", H, F, &L.wq_d}};
        for (const auto &t : proj) {
            *t.q = QuantW{};
            const char *bound = nullptr;
            for (const WqFormat &f : WQ_FORMATS) {
                const std::string cn = p + t.n + f.codes_sfx, sn = p + t.n + f.scales_sfx;
                if (!c->w.count(cn) && !c->w.count(sn)) continue;
                if (t.N % 16 || t.K % 64) return fail(OPUS_ESHAPE, "weight '%s': %s panels need N %% 16 == 0 and K %% 64 == 0", cn.c_str(), f.name);
                if (bound) return fail(OPUS_EBADARG, "weight '%s%s': bound as %s and as %s panels", p.c_str(), t.n, bound, f.name);
                GW(cn, f.codes_dtype, (std::vector<int64_t>{t.N, t.K / f.codes_kdiv}), t.q->codes);
                GW(sn, f.scales_dtype, (f.scales_kdiv ? std::vector<int64_t>{t.N, t.K / f.scales_kdiv} : std::vector<int64_t>{t.N}), t.q->scales);
                t.q->fmt = f.fmt;
                bound = f.name;
            }
        }
    }
    if (g.dec_arch == 1) {
        GW("dec.pos", OPUS_F16, (std::vector<int64_t>{g.dec_max_pos + 2, H}), c->dec_pos);
        GW("dec.lnf.w", OPUS_F32, (std::vector<int64_t>{H}), c->dec_lnfw);
        GW("dec.lnf.b", OPUS_F32, (std::vector<int64_t>{H}), c->dec_lnfb);
    }
    GW("dec.lm_head", OPUS_F16, (std::vector<int64_t>{V, H}), c->lm_head);
    c->resolved = true;
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ launch helpers
// Per-launch timing (timing mode only): the principal kernel of the bracketed call is dispatched with its own start /
// end events (OPUS_LAUNCH), a split-K reduce behind it with a second pair; a call that launches through plain
// hipLaunchKernelGGL falls back to events recorded around it on the stream.
struct Timed {
    opus_ctx *c;
    hipStream_t s;
    int klass;
    double bytes, flops;
    LaunchEvents ev;
    hipEvent_t b0 = nullptr, b1 = nullptr;
    Timed(opus_ctx *c_, hipStream_t s_, int k, double b, double f = 0.0) : c(c_), s(s_), klass(k), bytes(b), flops(f) {
        if (c->timing) {
            (void)hipEventCreate(&ev.main0); (void)hipEventCreate(&ev.main1);
            (void)hipEventCreate(&ev.aux0); (void)hipEventCreate(&ev.aux1);
            (void)hipEventCreate(&b0); (void)hipEventCreate(&b1);
            (void)hipEventRecord(b0, s);
            tl_launch_ev = &ev;
        }
    }
    ~Timed() {
        if (!c->timing) return;
        tl_launch_ev = nullptr;
        if (ev.main_used) {
            c->recs.push_back(TimeRec{ev.main_class >= 0 ? ev.main_class : klass, c->phase, ev.main0, ev.main1, bytes, flops});
            (void)hipEventDestroy(b0); (void)hipEventDestroy(b1);
        } else {
            (void)hipEventRecord(b1, s);
            c->recs.push_back(TimeRec{klass, c->phase, b0, b1, bytes, flops});
            (void)hipEventDestroy(ev.main0); (void)hipEventDestroy(ev.main1);
        }
        if (ev.aux_used) c->recs.push_back(TimeRec{KC_REDUCE, c->phase, ev.aux0, ev.aux1, ev.aux_bytes, 0.0});
        else { (void)hipEventDestroy(ev.aux0); (void)hipEventDestroy(ev.aux1); }
    }
};

// What one GEMM call asks for beyond shape, operands and epilogue (the fusion fields of GemmParams), built in the statement of the
// call: GemmAsk().copy16(c->d_xln).tiled_a(wo_tiled).  The defaults ask for nothing.
struct GemmAsk {
    half_t *xh = nullptr;                // row-scale producer: fp16 copy of the output here, sums of squares of its rows into d_ssq
    int xh_tiled = 0;                    //   ... the copy in fragment order
    bool rs_on = false;                  // row-scale consumer: rows times the rstd from d_ssq (rs_nblk blocks per row, as the
    float rs_eps = 0.f;                  //   producer reported them)
    int rs_nblk = 0;
    const float *rope_cs = nullptr;      // ESM rotary in the epilogue (GemmParams::rope_*)
    const int32_t *rope_pos = nullptr;
    int rope_T = 0, rope_cols = 0, rope_qcols = 0;
    float rope_qscale = 1.0f;
    float *ln_part = nullptr;            // fused-norm producer (GemmParams::ln_*): partials here, fp16(x) into ln_xh; takes
    half_t *ln_xh = nullptr;             //   precedence over the row-scale producer
    const float *ln_stat = nullptr, *ln_colsum = nullptr;   // fused-norm consumer
    int force_wide = 0, slab_only = 0;   // route a narrow output through the wide kernel / leave raw k-part slabs
    int a_tiled = 0, c_tiled = 0;        // A is read / the fp16 output is written in fragment order
    int *pp_plan = nullptr;              // (HOST) launch_pp reports its plan here
    QuantW wq;                           // quantised form of W (GemmParams::wq): streamed by a kernel that has an instantiation
                                         //   for its format, ignored by every other one (W holds the same values)
    // setters; a null first pointer leaves that request unasked
    GemmAsk &copy16(half_t *dst, bool tiled = false) { xh = dst; xh_tiled = dst && tiled; return *this; }
    GemmAsk &scale_rows(float eps, int nblk) { rs_on = true; rs_eps = eps; rs_nblk = nblk; return *this; }
    GemmAsk &rope(const float *cs, const int32_t *pos, int T, int D, float qscale) {   // the q and k thirds of [q k v] x D, q scaled
        if (cs) { rope_cs = cs; rope_pos = pos; rope_T = T; rope_cols = 2 * D; rope_qcols = D; rope_qscale = qscale; }
        return *this;
    }
    GemmAsk &ln_produce(float *part, half_t *x16) { if (part) { ln_part = part; ln_xh = x16; } return *this; }
    GemmAsk &ln_consume(const float *stat, const float *colsum) { if (stat) { ln_stat = stat; ln_colsum = colsum; } return *this; }
    GemmAsk &slabs() { force_wide = slab_only = 1; return *this; }
    GemmAsk &tiled_a(int on) { a_tiled = on; return *this; }
    GemmAsk &tiled_c(int on) { c_tiled = on; return *this; }
    GemmAsk &report_pp(int *plan) { pp_plan = plan; return *this; }
    GemmAsk &quant(const QuantW &q) { if (q.fmt != WQ_NONE && q.codes && q.scales) wq = q; return *this; }
};
// What the launch reports back: the row-scale producer's copy was written (ssq_nblk blocks of sums of squares per row), the rotary
// ran in the epilogue, the norm partials were written; ks > 1: that many raw k-part slabs were left (slab_only).
struct GemmGot {
    int xh_done = 0, rope_done = 0, ln_done = 0, ks = 1, ssq_nblk = 0;
};

static int gemm_any(opus_ctx *c, hipStream_t s, const half_t *A, const float *Af, float eps, int64_t lda, const half_t *W,
                    int M, int N, int K, const float *bias, int epi, const float *residual, void *C, int64_t ldc,
                    int out_f32, const GemmAsk &ask = GemmAsk(), GemmGot *got = nullptr) {
    GemmGot mine;
    if (!got) got = &mine;
    *got = GemmGot();
    GemmParams p;
    p.A = A; p.Af = Af; p.norm_eps = eps; p.lda = lda; p.W = W; p.M = M; p.N = N; p.K = K; p.bias = bias;
    p.residual = residual; p.ldr = ldc; p.C = C; p.ldc = ldc; p.out_f32 = out_f32; p.epi = epi;
    p.ws = c->gemm_ws; p.ws_bytes = c->gemm_ws_bytes;
    p.xh_out = ask.xh; p.ssq_out = c->d_ssq; p.fused_done = &got->xh_done; p.ssq_cap = c->ssq_cap; p.nblk_out = &got->ssq_nblk;
    p.rope_cs = ask.rope_cs; p.rope_T = ask.rope_T; p.rope_cols = ask.rope_cols; p.rope_qcols = ask.rope_qcols;
    p.rope_qscale = ask.rope_qscale; p.rope_done = &got->rope_done; p.rope_pos = ask.rope_pos;
    p.row_ssq = nullptr; p.row_nblk = 0;
    if (ask.rs_on) { p.row_ssq = c->d_ssq; p.row_nblk = ask.rs_nblk; p.norm_eps = ask.rs_eps; }
    p.force_wide = ask.force_wide; p.slab_only = ask.slab_only; p.ks_out = &got->ks;
    if (ask.ln_part) { p.xh_out = ask.ln_xh; p.ssq_out = nullptr; p.ln_part = ask.ln_part; p.ln_done = &got->ln_done; }
    if (ask.ln_stat) { p.ln_stat = ask.ln_stat; p.ln_colsum = ask.ln_colsum; }
    p.combine_cnt = c->d_cnt;
    p.pp_plan = ask.pp_plan;
    for (int i = 0; i < GEMM_PLAN_WORDS; ++i) c->gemm_plan[i] = -1;
    p.plan = c->gemm_plan;
    c->gemm_wq = WQ_NONE;
    p.wq = ask.wq; p.ran_wq = &c->gemm_wq;
    p.a_tiled = ask.a_tiled; p.xh_tiled = ask.xh_tiled; p.c_tiled = ask.c_tiled;
    const int nout = epi == EPI_SILU_GU16 ? N / 2 : N;
    // algorithmic bytes: the weights once + activations in + result out (+ the residual read)
    const double bytes = 2.0 * N * K + (Af ? 4.0 : 2.0) * M * K + (double)M * nout * (out_f32 ? 4 : 2) +
                         (residual ? 4.0 * M * nout : 0.0);
    int klass = M <= SKINNY_MAX_M ? KC_SKINNY : KC_TILE;
    hipError_t e;
    {
        Timed t(c, s, klass, bytes, 2.0 * M * N * (double)K);
        e = launch_gemm(p, s, &klass);
    }
    if (e != hipSuccess) return fail(OPUS_EHIP, "gemm M=%d N=%d K=%d failed: %s", M, N, K, hipGetErrorString(e));
    if (c->gemm_wq != WQ_NONE) ++c->wq_gemms[c->gemm_wq];
    return OPUS_OK;
}
static int gemm(opus_ctx *c, hipStream_t s, const half_t *A, int64_t lda, const half_t *W, int M, int N, int K,
                const float *bias, int epi, const float *residual, void *C, int64_t ldc, int out_f32,
                const GemmAsk &ask = GemmAsk(), GemmGot *got = nullptr) {
    return gemm_any(c, s, A, nullptr, 0.f, lda, W, M, N, K, bias, epi, residual, C, ldc, out_f32, ask, got);
}
// The shadow of the residual stream inside one prefill / decode step: which fp32 buffer currently has a valid fp16 copy (d_xn /
// d_xln) with the sums of squares of its rows in d_ssq.  A producer GEMM sets it from its outcome, every gemm_norm() consumes it.
struct ResidShadow {
    const float *xh_src = nullptr;       // fp32 buffer whose fp16 copy + sum-of-squares partials are valid
    int ssq_nblk = 0;                    // blocks per row the producer wrote (N / 256: split-K reduce, embedding; N / 16: gemm_stream)
    bool xln_tiled = false;              // d_xln holds that copy in fragment order
    void produced(const float *x, const GemmGot &got, bool tiled = false) {
        xh_src = got.xh_done ? x : nullptr;
        if (got.xh_done) ssq_nblk = got.ssq_nblk;
        xln_tiled = got.xh_done && tiled;
    }
};
static bool fuse_rows() {
    static const bool off = getenv("OPUS_NO_ROW_FUSION") != nullptr;   // A/B aid
    return !off;
}
#define KLF(klass, bytes, flops, call)                                                                \
    do {                                                                                              \
        hipError_t e_;                                                                                \
        {                                                                                             \
            Timed t_(c, s, klass, bytes, flops);                                                      \
            e_ = (call);                                                                              \
        }                                                                                             \
        if (e_ != hipSuccess) return fail(OPUS_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define KL(klass, bytes, call) KLF(klass, bytes, 0.0, call)

// C = epi(rmsnorm(X) W'^T) with the norm weight pre-folded into W': fused in the skinny kernel (M <= 64),
// otherwise a weight-less rmsnorm kernel into `scratch` followed by the tile kernel.  Consumes the shadow; `ask` goes to the
// one GEMM that runs.
static int gemm_norm(opus_ctx *c, hipStream_t s, ResidShadow &sh, const float *X, float eps, half_t *scratch, const half_t *W, int M,
                     int N, int K, int epi, void *C, int64_t ldc, int out_f32, const float *bias = nullptr,
                     const GemmAsk &ask = GemmAsk(), GemmGot *got = nullptr) {
    static const bool no_mid = getenv("OPUS_NO_MID_GEMM") != nullptr;
    static const bool mid_v1 = getenv("OPUS_MID_V1") != nullptr;
    const bool shadowed = sh.xh_src == X;
    sh.xh_src = nullptr;
    if (shadowed && bias == nullptr && (K & 255) == 0 && gemm_goes_wide(M, N))
        // the producer's split-K reduce left fp16(X) in `scratch` and per-block sums of squares: no norm launch, the
        // wide kernel scales its rows instead
        return gemm(c, s, scratch, K, W, M, N, K, nullptr, epi, nullptr, C, ldc, out_f32, GemmAsk(ask).scale_rows(eps, sh.ssq_nblk), got);
    // 17..64 rows with a wide output (wgu, lm_head): the wide kernel wants fp16 activations, so norm separately
    const bool wide = M > SKINNY_MAX_M && N >= 16384 && !mid_v1;
    if (M <= SKINNY_MAX_M || (M <= MID_MAX_M && !no_mid && !wide))
        return gemm_any(c, s, nullptr, X, eps, K, W, M, N, K, bias, epi, nullptr, C, ldc, out_f32, ask, got);
    KL(KC_NORM, 6.0 * M * K, launch_rmsnorm(X, nullptr, eps, M, K, scratch, s));
    return gemm(c, s, scratch, K, W, M, N, K, bias, epi, nullptr, C, ldc, out_f32, ask, got);
}

static int need_ready(opus_ctx *c) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    OPC(opus_weights_ready(c));
    HIPC(hipSetDevice(c->device));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ load-time ops
extern "C" int opus_lora_merge(void *W, const void *A, const void *B, float scale, int64_t out_f, int64_t in_f,
                               int32_t r, void *stream) {
    if (!W || !A || !B || out_f < 1 || in_f < 1 || r < 1) return fail(OPUS_EBADARG, "lora_merge: bad argument");
    if (in_f % 8) return fail(OPUS_ESHAPE, "lora_merge: in_features must be a multiple of 8");
    HIPC(launch_lora_merge((half_t *)W, (const half_t *)A, (const half_t *)B, scale, out_f, in_f, r, (hipStream_t)stream));
    return OPUS_OK;
}

extern "C" int opus_fill_synth(void *dst, int dtype, int64_t rows, int64_t cols, uint64_t seed, float std, float mean,
                               int64_t row_block, int64_t row_stride, int64_t row_off, int32_t tiled, uint64_t fold_seed,
                               float fold_std, float fold_mean, void *stream) {
    if (!dst || rows < 1 || cols < 1 || (dtype != OPUS_F16 && dtype != OPUS_F32) || row_block < 1 || row_stride < row_block)
        return fail(OPUS_EBADARG, "fill_synth: bad argument");
    if (tiled && (cols % 64 || row_block % 16 || row_stride % 16 || row_off % 16))
        return fail(OPUS_ESHAPE, "fill_synth: tiled layout needs cols %% 64 == 0 and 16-row aligned blocks");
    HIPC(launch_fill_synth(dst, dtype, rows, cols, seed, std, mean, row_block, row_stride, row_off, tiled ? 1 : 0,
                           fold_seed, fold_std, fold_mean, (hipStream_t)stream));
    return OPUS_OK;
}

extern "C" int opus_tile_weight(const void *d_src, void *d_dst, int64_t N, int64_t K, void *stream) {
    if (!d_src || !d_dst || d_src == d_dst) return fail(OPUS_EBADARG, "tile_weight: null or aliased pointers");
    if (N < 16 || K < 64 || N % 16 || K % 64) return fail(OPUS_ESHAPE, "tile_weight: N %% 16 == 0 and K %% 64 == 0 required");
    HIPC(launch_tile_weight((const half_t *)d_src, (half_t *)d_dst, N, K, (hipStream_t)stream));
    return OPUS_OK;
}

// Quantised form of one decoder-layer weight (csrc/quant.hip): the checks, the `bad` word, the synchronisation and the error
// reporting of opus_quantize_fp8 / opus_quantize_mxfp4; `launch(d_bad, s)` starts the format's kernel, `aligned` are the pointers
// that must be 16-byte aligned.
template <class Launch>
static int quantize_any(const char *who, const void *d_src, int64_t N, int64_t K, const void *d_codes, const void *d_scales,
                        uintptr_t aligned, void *stream, Launch launch) {
    if (!d_src || !d_codes || !d_scales) return fail(OPUS_EBADARG, "%s: null pointer", who);
    if (N < 16 || K < 64 || N % 16 || K % 64) return fail(OPUS_ESHAPE, "%s: N %% 16 == 0 and K %% 64 == 0 required", who);
    if (aligned & 15) return fail(OPUS_EBADARG, "%s: pointers must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    int *d_bad = nullptr;
    HIPC(hipMalloc(&d_bad, sizeof(int)));
    int bad = 0;
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), s);
    if (e == hipSuccess) e = launch(d_bad, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return fail(OPUS_EHIP, "%s failed: %s", who, hipGetErrorString(e));
    if (bad) return fail(OPUS_EBADARG, "%s: the weight holds a value that is not finite", who);
    return OPUS_OK;
}

// FP8: row-major W[N, K] in the operand type -> q8 (FP8 panels, N K bytes), e8 (int8 [N]) and, when d_dq is not null, the
// dequantised weights (operand type, row-major [N, K]; may be d_src itself).
// Synchronises the stream: a weight that is not finite is reported (OPUS_EBADARG) and the outputs are not to be used.
extern "C" int opus_quantize_fp8(const void *d_src, int64_t N, int64_t K, void *d_q8, void *d_e8, void *d_dq, void *stream) {
    return quantize_any("quantize_fp8", d_src, N, K, d_q8, d_e8, (uintptr_t)d_src | (uintptr_t)d_q8 | (uintptr_t)d_dq, stream,
                        [&](int *d_bad, hipStream_t s) {
        return launch_quantize_fp8((const half_t *)d_src, N, K, (uint8_t *)d_q8, (int8_t *)d_e8, (half_t *)d_dq, d_bad, s);
    });
}

// MXFP4: -> q4 (code panels, N K / 2 bytes), s4 (scale panels, N K / 32 bytes) and the dequantised weights, on the same terms.
extern "C" int opus_quantize_mxfp4(const void *d_src, int64_t N, int64_t K, void *d_q4, void *d_s4, void *d_dq, void *stream) {
    return quantize_any("quantize_mxfp4", d_src, N, K, d_q4, d_s4,
                        (uintptr_t)d_src | (uintptr_t)d_q4 | (uintptr_t)d_s4 | (uintptr_t)d_dq, stream, [&](int *d_bad, hipStream_t s) {
        return launch_quantize_mxfp4((const half_t *)d_src, N, K, (uint8_t *)d_q4, (uint8_t *)d_s4, (half_t *)d_dq, d_bad, s);
    });
}

// ------------------------------------------------------------------------------------------------ encoder
// The encoder over M token rows.  Padded form (d_cu == nullptr): M = B T rows, row b t at b T + t, keys >= lens[b] masked.
// Token-packed form (SURVEY 5 "length-bucketed / varlen batches"): the rows are the proteins' tokens back to back, d_cu[B + 1] their
// offsets, T the longest protein - the GEMMs multiply no padding and a batch of mixed lengths is ONE set of large launches
// instead of one per length bucket; positions come from a row -> position table (written by the embedding kernel), the attention
// takes its rows from cu.
// Contact maps riding along the packed encoder (opus_esm2_contacts_packed): the regression head and the caller-scratch buffers
// (contact.hip's layouts), n_max = the longest protein's interior length.
struct ContactRun {
    const float *w, *bias;
    float *A, *vec, *part, *sw, *out;
    int n_max;
};

static int contact_layer(opus_ctx *c, hipStream_t s, const ContactRun &ct, int l, int B) {
    const opus_config &g = c->cfg;
    const int D = g.enc_dim, nh = g.enc_heads, hd = D / nh, C = g.enc_layers * nh;
    ContactParams p;
    p.Q = c->e_qkv; p.K = c->e_qkv + D; p.ld = 3 * D; p.cu = c->e_cu; p.B = B; p.heads = nh; p.w = ct.w + l * nh;
    p.A = ct.A; p.accumulate = l > 0; p.rows = ct.vec; p.vld = C; p.c0 = l * nh; p.part = ct.part;
    double n2 = 0.0, nt = 0.0;                                       // (interior n^2, all-key T n per protein)
    for (int b = 0; b < B; ++b) {
        const double n = c->h_cu[b + 1] - c->h_cu[b] - 2, t = n + 2;
        if (n > 0) { n2 += n * n; nt += n * t; }
    }
    // two Q K^T passes over every head; bytes: the A tile read-modify-write + Q / K once
    KLF(KC_CONTACT, 8.0 * n2 + 4.0 * (c->h_cu[B]) * D, 2.0 * 2.0 * nt * hd * nh, launch_esm_contact_accum(p, hd, ct.n_max, s));
    KL(KC_CONTACT, 4.0 * n2 / 64.0 * nh * 2.0, launch_esm_contact_colsum(ct.part, c->e_cu, B, nh, ct.n_max, ct.vec, C, l * nh, 1, s));
    return OPUS_OK;
}

static int esm2_encode_rows(opus_ctx *c, hipStream_t s, const int32_t *d_tokens, const int32_t *d_lens, const int32_t *d_cu, int B, int T,
                            int M, float *d_pooled, const ContactRun *ct = nullptr) {
    const opus_config &g = c->cfg;
    c->phase = PH_ENCODE;
    c->enc_rows = 0;                               // (e_hid is being rewritten: valid again when every launch below was enqueued)
    const int D = g.enc_dim, F = g.enc_ffn, nh = g.enc_heads, hd = D / nh;
    const bool packed = d_cu != nullptr;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_ERR * sizeof(int32_t), s));       // hand-off words start from zero on every call
    if (packed) KL(KC_OTHER, 4.0 * M * D, launch_esm_embed_packed(d_tokens, c->enc_emb, d_cu, B, T, D, c->e_x, c->e_pos, s));
    else KL(KC_OTHER, 4.0 * M * D, launch_esm_embed(d_tokens, c->enc_emb, B, T, D, c->e_x, s));
    // Pre-LN blocks with the LayerNorm fused around the big tiled GEMM (GemmParams::ln_*): the epilogue that writes
    // the residual stream (wo, fc2) also leaves fp16(x) and per-row partial sums, a small kernel turns those into (mu, rstd),
    // and the consuming projection (fc1, the next layer's QKV) runs on fp16(x) as it stands and applies
    // rstd (acc - mu s) + c2 in its epilogue - no pass over the fp32 stream in between.  Shapes the big kernel does not take
    // (few rows), the first layer, and OPUS_NO_LN_FUSION=1 use the stand-alone normalisation (x - mu) rstd (the affine part
    // lives in the folded weights either way).
    static const bool no_ln_env = getenv("OPUS_NO_LN_FUSION") != nullptr;      // A/B aid (also the knob of the same name)
    const bool no_ln_fusion = no_ln_env || g_knobs.no_ln_fusion;
    const bool qkv_pp = !no_ln_fusion && (D & 255) == 0 && gemm_goes_pp(M, 3 * D);
    const bool fc1_pp = !no_ln_fusion && (D & 255) == 0 && gemm_goes_pp(M, F);
    bool have_stat = false;                        // e_xn = fp16(x), e_stat = (mu, rstd) of the current residual stream
    auto finalize = [&]() -> int {
        KL(KC_NORM, 8.0 * M * (D / 64) + 8.0 * M, launch_ln_finalize(c->e_part, M, D / 64, D, g.enc_ln_eps, 0, c->e_stat, s));
        return OPUS_OK;
    };
    double attn_flops = 0.0;                       // 4 T_b^2 D per protein
    if (packed) for (int b = 0; b < B; ++b) { const double t = c->h_cu[b + 1] - c->h_cu[b]; attn_flops += 4.0 * t * t * D; }
    else attn_flops = 4.0 * B * (double)T * T * D;
    for (int l = 0; l < g.enc_layers; ++l) {
        const EncLayer &L = c->enc[l];
        GemmAsk qkv;
        GemmGot got;
        if (have_stat && qkv_pp) qkv.ln_consume(c->e_stat, L.sqkv);
        else KL(KC_NORM, 6.0 * M * D, launch_layernorm(c->e_x, nullptr, nullptr, g.enc_ln_eps, M, D, c->e_xn, nullptr, s));
        // q <- rotary(q * hd^-0.5), k <- rotary(k): in the projection's epilogue when the big tiled kernel takes it (head_dim 64),
        // else by the stand-alone kernel on the stored projection (same arithmetic)
        if (hd == 64) qkv.rope(c->cs_enc, packed ? c->e_pos : nullptr, packed ? g.max_enc_tokens : T, D, 1.0f / sqrtf((float)hd));
        OPC(gemm(c, s, c->e_xn, D, L.wqkv, M, 3 * D, D, L.bqkv, EPI_NONE, nullptr, c->e_qkv, 3 * D, 0, qkv, &got));
        if (!got.rope_done) {
            if (packed) KL(KC_OTHER, 8.0 * M * D, launch_esm_rope(c->e_qkv, c->cs_enc, 1, M, nh, hd, 1.0f / sqrtf((float)hd), s, c->e_pos));
            else KL(KC_OTHER, 8.0 * M * D, launch_esm_rope(c->e_qkv, c->cs_enc, B, T, nh, hd, 1.0f / sqrtf((float)hd), s));
        }
        if (ct) OPC(contact_layer(c, s, *ct, l, B));                 // (e_qkv: q scaled and rotated, k rotated, every token row)
        AttnParams a;
        a.Q = c->e_qkv; a.K = c->e_qkv + D; a.V = c->e_qkv + 2 * D;
        a.q_sb = a.k_sb = a.v_sb = packed ? 0 : (int64_t)T * 3 * D;
        a.q_st = a.k_st = a.v_st = 3 * D;
        a.O = c->e_ctx; a.o_sb = packed ? 0 : (int64_t)T * D; a.o_st = D;
        a.kstart = nullptr; a.kend = packed ? nullptr : d_lens; a.cu = d_cu;
        a.B = B; a.T = T; a.heads = nh; a.group = 1; a.head_dim = hd; a.causal = 0; a.scale = 1.0f;
        // last layer: the <cls> / <eos> rows of representations[L] are dropped by the mean-pool (cstp_v3/modelling.py:52-54): they
        // are keys but not queries (512 residues: four query blocks instead of five).  The debug tap opus_esm2_last_hidden then
        // holds no representation in those rows; knob "enc_full_last_layer" = 1 computes them (parity tests of every token's state).
        a.q_trim = packed && l + 1 == g.enc_layers && T > 2 && !g_knobs.enc_full_last_layer ? 1 : 0;
        KLF(KC_ATTN_PREFILL, 8.0 * M * D, attn_flops, launch_attn_prefill(a, s));
        OPC(gemm(c, s, c->e_ctx, D, L.wo, M, D, D, L.bo, EPI_NONE, c->e_x, c->e_x, D, 1, GemmAsk().ln_produce(fc1_pp ? c->e_part : nullptr, c->e_xn), &got));
        have_stat = got.ln_done != 0;
        if (have_stat) OPC(finalize());
        else KL(KC_NORM, 6.0 * M * D, launch_layernorm(c->e_x, nullptr, nullptr, g.enc_ln_eps, M, D, c->e_xn, nullptr, s));
        OPC(gemm(c, s, c->e_xn, D, L.w1, M, F, D, L.b1, EPI_GELU, nullptr, c->e_h1, F, 0, GemmAsk().ln_consume(have_stat ? c->e_stat : nullptr, L.s1)));
        const bool next_pp = qkv_pp && l + 1 < g.enc_layers;
        OPC(gemm(c, s, c->e_h1, F, L.w2, M, D, F, L.b2, EPI_NONE, c->e_x, c->e_x, D, 1, GemmAsk().ln_produce(next_pp ? c->e_part : nullptr, c->e_xn), &got));
        have_stat = got.ln_done != 0;
        if (have_stat) OPC(finalize());
    }
    KL(KC_NORM, 8.0 * M * D, launch_layernorm(c->e_x, c->enc_lnfw, c->enc_lnfb, g.enc_ln_eps, M, D, nullptr, c->e_hid, s));
    if (packed) KL(KC_OTHER, 4.0 * M * D, launch_masked_mean_packed(c->e_hid, d_cu, B, D, d_pooled, s));
    else KL(KC_OTHER, 4.0 * M * D, launch_masked_mean(c->e_hid, d_lens, B, T, D, d_pooled, s));
    if (ct) {
        const int C = g.enc_layers * nh;
        double n2 = 0.0, ni = 0.0;
        for (int b = 0; b < B; ++b) { const double n = c->h_cu[b + 1] - c->h_cu[b] - 2; n2 += n * n; ni += n; }
        KL(KC_CONTACT, 4.0 * ni * C, launch_esm_contact_scale(ct->vec, d_cu, B, C, ct->w, ct->sw, s));
        KLF(KC_CONTACT, 12.0 * n2 + 8.0 * ni * C * cdiv((int64_t)ct->n_max, 64), 2.0 * n2 * C,
            launch_esm_contact_finish(ct->A, ct->vec, ct->sw, d_cu, B, C, ct->n_max, ct->bias, ct->out, s));
    }
    c->enc_rows = M;
    return OPUS_OK;
}

extern "C" int opus_esm2_encode(opus_ctx *c, const int32_t *d_tokens, const int32_t *d_lens, int32_t B, int32_t T,
                                float *d_pooled, void *stream) {
    OPC(need_ready(c));
    if (!d_tokens || !d_lens || !d_pooled) return fail(OPUS_EBADARG, "esm2_encode: null pointer");
    const opus_config &g = c->cfg;
    if (B < 1 || B > g.max_batch || T < 3 || T > g.max_enc_tokens)
        return fail(OPUS_ESHAPE, "esm2_encode: B=%d T=%d exceed capacity (%d, %d)", B, T, g.max_batch, g.max_enc_tokens);
    return esm2_encode_rows(c, (hipStream_t)stream, d_tokens, d_lens, nullptr, B, T, B * T, d_pooled);
}

extern "C" int opus_esm2_encode_packed(opus_ctx *c, const int32_t *d_tokens, const int32_t *h_cu, int32_t B, float *d_pooled,
                                       void *stream) {
    OPC(need_ready(c));
    if (!d_tokens || !h_cu || !d_pooled) return fail(OPUS_EBADARG, "esm2_encode_packed: null pointer");
    const opus_config &g = c->cfg;
    if (B < 1 || B > g.max_batch) return fail(OPUS_ESHAPE, "esm2_encode_packed: B=%d exceeds max_batch=%d", B, g.max_batch);
    if (h_cu[0] != 0) return fail(OPUS_EBADARG, "esm2_encode_packed: cu[0] must be 0");
    int Tmax = 0;
    for (int b = 0; b < B; ++b) {
        const int t = h_cu[b + 1] - h_cu[b];
        if (t < 2 || t > g.max_enc_tokens)     // (<cls> <eos> at least)
            return fail(OPUS_ESHAPE, "esm2_encode_packed: protein %d has %d tokens (2 .. max_enc_tokens=%d)", b, t, g.max_enc_tokens);
        Tmax = t > Tmax ? t : Tmax;
    }
    const int64_t M = h_cu[B];
    if (M > (int64_t)g.max_batch * g.max_enc_tokens) return fail(OPUS_ESHAPE, "esm2_encode_packed: %lld tokens exceed the workspace", (long long)M);
    hipStream_t s = (hipStream_t)stream;
    c->h_cu.assign(h_cu, h_cu + B + 1);                              // (host copy: per-protein FLOP accounting of the timing records)
    HIPC(launch_upload_i32(h_cu, B + 1, c->e_cu, s));                 // through the kernel arguments: no host buffer outlives the call
    return esm2_encode_rows(c, s, d_tokens, nullptr, c->e_cu, B, Tmax, (int)M, d_pooled);
}

// ------------------------------------------------------------------------------------------------ contact maps
// Caller scratch of opus_esm2_contacts_packed (contact.hip layouts): A [sum n^2] | vec [sum n][C] | part [H sum cdiv(n, 64) n] |
// sw [B][C] fp32, each 256-byte aligned.  n = tokens - 2 per protein.
struct ContactScratch {
    int64_t a, vec, part, sw, total;
    int n_max;
};
static ContactScratch contact_scratch(const opus_config &g, const int32_t *h_cu, int B) {
    ContactScratch z{};
    const int64_t C = (int64_t)g.enc_layers * g.enc_heads;
    int64_t n2 = 0, ni = 0, pq = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = std::max<int64_t>(h_cu[b + 1] - h_cu[b] - 2, 0);
        n2 += n * n; ni += n; pq += (n + 63) / 64 * n;
        z.n_max = std::max<int>(z.n_max, (int)n);
    }
    z.a = 0;
    z.vec = z.a + (int64_t)align_up((size_t)n2 * 4);
    z.part = z.vec + (int64_t)align_up((size_t)(ni * C) * 4);
    z.sw = z.part + (int64_t)align_up((size_t)(pq * g.enc_heads) * 4);
    z.total = z.sw + (int64_t)align_up((size_t)(B * C) * 4);
    return z;
}

static int check_packed_cu(const opus_config &g, const int32_t *h_cu, int B, const char *who) {
    if (B < 1 || B > g.max_batch) return fail(OPUS_ESHAPE, "%s: B=%d exceeds max_batch=%d", who, B, g.max_batch);
    if (h_cu[0] != 0) return fail(OPUS_EBADARG, "%s: cu[0] must be 0", who);
    for (int b = 0; b < B; ++b) {
        const int t = h_cu[b + 1] - h_cu[b];
        if (t < 2 || t > g.max_enc_tokens)
            return fail(OPUS_ESHAPE, "%s: protein %d has %d tokens (2 .. max_enc_tokens=%d)", who, b, t, g.max_enc_tokens);
    }
    if (h_cu[B] > (int64_t)g.max_batch * g.max_enc_tokens) return fail(OPUS_ESHAPE, "%s: %d tokens exceed the workspace", who, h_cu[B]);
    return OPUS_OK;
}

extern "C" int64_t opus_esm2_contacts_scratch_bytes(const opus_config *cfg, const int32_t *h_cu, int32_t B) {
    if (!cfg || !h_cu || check_cfg(cfg) != OPUS_OK || check_packed_cu(*cfg, h_cu, B, "esm2_contacts_scratch_bytes") != OPUS_OK) return -1;
    return contact_scratch(*cfg, h_cu, B).total;
}

extern "C" int opus_esm2_contacts_packed(opus_ctx *c, const int32_t *d_tokens, const int32_t *h_cu, int32_t B, float *d_pooled,
                                         float *d_contacts, void *d_scratch, int64_t scratch_bytes, void *stream) {
    OPC(need_ready(c));
    if (!d_tokens || !h_cu || !d_pooled || !d_contacts || !d_scratch) return fail(OPUS_EBADARG, "esm2_contacts_packed: null pointer");
    const opus_config &g = c->cfg;
    OPC(check_packed_cu(g, h_cu, B, "esm2_contacts_packed"));
    const int64_t C = (int64_t)g.enc_layers * g.enc_heads;
    ContactRun ct;
    GW("enc.contact.weight", OPUS_F32, (std::vector<int64_t>{C}), ct.w);
    GW("enc.contact.bias", OPUS_F32, (std::vector<int64_t>{1}), ct.bias);
    const ContactScratch z = contact_scratch(g, h_cu, B);
    if (scratch_bytes < z.total)
        return fail(OPUS_ESHAPE, "esm2_contacts_packed: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)z.total);
    if (((uintptr_t)d_scratch) & 255) return fail(OPUS_EBADARG, "esm2_contacts_packed: scratch must be 256-byte aligned");
    char *base = (char *)d_scratch;
    ct.A = (float *)(base + z.a); ct.vec = (float *)(base + z.vec); ct.part = (float *)(base + z.part); ct.sw = (float *)(base + z.sw);
    ct.out = d_contacts;
    ct.n_max = z.n_max;
    int Tmax = 0;
    for (int b = 0; b < B; ++b) Tmax = std::max(Tmax, h_cu[b + 1] - h_cu[b]);
    hipStream_t s = (hipStream_t)stream;
    c->h_cu.assign(h_cu, h_cu + B + 1);
    HIPC(launch_upload_i32(h_cu, B + 1, c->e_cu, s));
    return esm2_encode_rows(c, s, d_tokens, nullptr, c->e_cu, B, Tmax, h_cu[B], d_pooled, &ct);
}

extern "C" int opus_debug_contacts(opus_ctx *c, const void *d_q, const void *d_k, int64_t ld, const int32_t *h_cu, int32_t B,
                                   int32_t heads, int32_t head_dim, const float *d_w, float *d_A, float *d_rows, float *d_cols,
                                   void *d_scratch, int64_t scratch_bytes, void *stream) {
    if (!c || !d_q || !d_k || !h_cu || !d_w || !d_A || !d_rows || !d_cols || !d_scratch) return fail(OPUS_EBADARG, "debug_contacts: null pointer");
    if (B < 1 || B > 4096 || heads < 1 || (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) || ld < (int64_t)heads * head_dim ||
        (ld & 7) || (((uintptr_t)d_q | (uintptr_t)d_k) & 15))
        return fail(OPUS_ESHAPE, "debug_contacts: B=%d heads=%d head_dim=%d ld=%lld", B, heads, head_dim, (long long)ld);
    if (contact_accum_lds(heads) > 160 * 1024) return fail(OPUS_ESHAPE, "debug_contacts: %d heads exceed the workgroup's LDS", heads);
    if (h_cu[0] != 0) return fail(OPUS_EBADARG, "debug_contacts: cu[0] must be 0");
    int64_t pq = 0;
    int n_max = 0;
    for (int b = 0; b < B; ++b) {
        const int t = h_cu[b + 1] - h_cu[b];
        if (t < 2) return fail(OPUS_ESHAPE, "debug_contacts: protein %d has %d tokens (at least 2)", b, t);
        pq += (int64_t)(t - 2 + 63) / 64 * (t - 2);
        n_max = std::max(n_max, t - 2);
    }
    const int64_t need = (int64_t)align_up((size_t)(B + 1) * 4) + pq * heads * 4;
    if (scratch_bytes < need) return fail(OPUS_ESHAPE, "debug_contacts: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int32_t *d_cu = (int32_t *)d_scratch;
    float *part = (float *)((char *)d_scratch + align_up((size_t)(B + 1) * 4));
    HIPC(launch_upload_i32(h_cu, B + 1, d_cu, s));
    ContactParams p;
    p.Q = (const half_t *)d_q; p.K = (const half_t *)d_k; p.ld = ld; p.cu = d_cu; p.B = B; p.heads = heads; p.w = d_w;
    p.A = d_A; p.accumulate = 0; p.rows = d_rows; p.vld = heads; p.c0 = 0; p.part = part;
    HIPC(launch_esm_contact_accum(p, head_dim, n_max, s));
    HIPC(launch_esm_contact_colsum(part, d_cu, B, heads, n_max, d_cols, heads, 0, 0, s));
    return OPUS_OK;
}

extern "C" int opus_esm2_last_hidden(opus_ctx *c, float *d_out, int32_t B, int32_t T, void *stream) {
    if (!c || !d_out) return fail(OPUS_EBADARG, "null pointer");
    if (B < 1 || T < 1 || (int64_t)B * T > (int64_t)c->cfg.max_batch * c->cfg.max_enc_tokens) return fail(OPUS_ESHAPE, "B/T out of range");   // (B = 1, T = all tokens: the packed form)
    HIPC(hipMemcpyAsync(d_out, c->e_hid, (size_t)B * T * c->cfg.enc_dim * sizeof(float), hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ masked-LM head
// logits = LN(gelu_erf(h Wd^T + bd)) We^T + b on R rows of `src` (the context's e_hid, or opus_debug_esm2_lm_head's copy in it):
// gather-and-cast into e_xn, the dense step through the GEMM router into e_h1 (erf-GELU epilogue, as fc1), mlm_head_kernel.
// Up to MLM_FIXED_ROWS rows the dense step is ONE launch shape (the operand padded with zero rows to that many): a row's logits
// then do not depend on how many other rows, or which, share the call - the masked scan's copies give the same bits however
// they are grouped - and the skinny / mid routes, whose summation orders differ, are not involved.  More rows: the router's
// choice for M = R.
constexpr int MLM_FIXED_ROWS = 128;
static const char *MLM_TENSORS = "enc.lm.dense.{weight,bias}, enc.lm.ln.{weight,bias}, enc.lm.bias (enc.lm.weight when untied)";

static int mlm_head_rows(opus_ctx *c, hipStream_t s, const float *src, int64_t src_rows, const int32_t *d_rows, int R,
                         int log_softmax, float *d_out) {
    const opus_config &g = c->cfg;
    const int64_t De = g.enc_dim, V = g.enc_vocab, Me = (int64_t)g.max_batch * g.max_enc_tokens;
    if (V > 64) return fail(OPUS_EUNSUPPORTED, "esm2_lm_head: enc_vocab=%d, at most 64 columns are built", g.enc_vocab);
    if (g.enc_ffn < g.enc_dim) return fail(OPUS_EUNSUPPORTED, "esm2_lm_head: enc_ffn < enc_dim (the dense step's output uses the fc1 buffer)");
    for (const char *n : {"enc.lm.dense.weight", "enc.lm.dense.bias", "enc.lm.ln.weight", "enc.lm.ln.bias", "enc.lm.bias"})
        if (!c->w.count(n)) return fail(OPUS_EBADARG, "esm2_lm_head: the masked-LM head is not bound ('%s' missing; it needs %s)", n, MLM_TENSORS);
    const half_t *wd, *we;
    const float *bd, *lw, *lb, *bv;
    GW("enc.lm.dense.weight", OPUS_F16, (std::vector<int64_t>{De, De}), wd);
    GW("enc.lm.dense.bias", OPUS_F32, (std::vector<int64_t>{De}), bd);
    GW("enc.lm.ln.weight", OPUS_F32, (std::vector<int64_t>{De}), lw);
    GW("enc.lm.ln.bias", OPUS_F32, (std::vector<int64_t>{De}), lb);
    GW("enc.lm.bias", OPUS_F32, (std::vector<int64_t>{V}), bv);
    if (c->w.count("enc.lm.weight")) GW("enc.lm.weight", OPUS_F16, (std::vector<int64_t>{V, De}), we);
    else we = c->enc_emb;                                            // tied to the token embedding, as fair-esm and transformers tie it
    const int fixed = (int)std::min<int64_t>(MLM_FIXED_ROWS, Me);
    const int Mg = R <= fixed ? fixed : R;
    const int saved_phase = c->phase;
    c->phase = PH_ENCODE;
    KL(KC_MLM, 6.0 * R * De, launch_mlm_gather(src, src_rows, d_rows, R, Mg, (int)De, c->e_xn, s));
    OPC(gemm(c, s, c->e_xn, De, wd, Mg, (int)De, (int)De, bd, EPI_GELU, nullptr, c->e_h1, De, 0));
    KLF(KC_MLM, 2.0 * R * De + 2.0 * V * De + 4.0 * R * V, 2.0 * R * V * De,
        launch_mlm_head(c->e_h1, lw, lb, g.enc_ln_eps, we, bv, R, (int)De, (int)V, log_softmax ? 1 : 0, d_out, s));
    c->phase = saved_phase;
    return OPUS_OK;
}

extern "C" int opus_esm2_lm_head(opus_ctx *c, const int32_t *d_rows, int32_t R, int32_t log_softmax, float *d_out, void *stream) {
    OPC(need_ready(c));
    if (!d_out) return fail(OPUS_EBADARG, "esm2_lm_head: null pointer");
    if (c->enc_rows < 1)
        return fail(OPUS_ESTATE, "esm2_lm_head: the context holds no encoder result (call opus_esm2_encode* / opus_esm2_contacts_packed first; "
                                 "opus_debug_esm2_lm_head overwrites it)");
    const int64_t Me = (int64_t)c->cfg.max_batch * c->cfg.max_enc_tokens;
    if (R < 1 || R > Me || (!d_rows && R > c->enc_rows))
        return fail(OPUS_ESHAPE, "esm2_lm_head: R=%d out of range (1 .. %lld; without a row list at most the %lld rows of the last encoder call)",
                    R, (long long)Me, (long long)c->enc_rows);
    return mlm_head_rows(c, (hipStream_t)stream, c->e_hid, c->enc_rows, d_rows, R, log_softmax, d_out);
}

extern "C" int opus_debug_esm2_lm_head(opus_ctx *c, const float *d_hidden, int32_t R, int32_t log_softmax, float *d_out, void *stream) {
    OPC(need_ready(c));
    if (!d_hidden || !d_out) return fail(OPUS_EBADARG, "debug_esm2_lm_head: null pointer");
    const int64_t Me = (int64_t)c->cfg.max_batch * c->cfg.max_enc_tokens;
    if (R < 1 || R > Me) return fail(OPUS_ESHAPE, "debug_esm2_lm_head: R=%d out of range (1 .. %lld)", R, (long long)Me);
    hipStream_t s = (hipStream_t)stream;
    c->enc_rows = 0;                                                 // the states go where the encoder leaves its own
    HIPC(hipMemcpyAsync(c->e_hid, d_hidden, (size_t)R * c->cfg.enc_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    return mlm_head_rows(c, s, c->e_hid, R, nullptr, R, log_softmax, d_out);
}

// ------------------------------------------------------------------------------------------------ projectors
// The projectors also serve the batched stage of the two-stage pipeline (whole shards at M >= 512; the 8H x 8H
// GEMM runs 1.18 / 1.30 / 1.34 PFLOP/s at 512 / 1024 / 4096 rows).  Its workspace (0.55 GB at the Llama-3-8B shape) is not
// part of every context: the first call that brings more rows than max_batch allocates it.
constexpr int BIG_PROJ_ROWS = 4096;
static int ensure_proj_rows(opus_ctx *c, int B) {
    if (B <= c->proj_rows || c->proj_big) return OPUS_OK;
    const opus_config &g = c->cfg;
    const size_t PR = BIG_PROJ_ROWS > g.max_batch ? BIG_PROJ_ROWS : g.max_batch;
    const size_t De = g.enc_dim, Dm = g.has_protein_projector ? g.proj_dim : g.enc_dim, SW = (size_t)g.dec_dim * g.n_prot_tokens;
    const size_t bytes = (align_up(PR * De * 2) + align_up(PR * Dm * 2) + 2 * align_up(PR * SW * 2));
    HIPC(hipMalloc((void **)&c->proj_big, bytes));
    Carver k{c->proj_big};
    c->p_xn = k.take<half_t>(PR * De);
    c->p_y = k.take<half_t>(PR * Dm);
    c->p_z[0] = k.take<half_t>(PR * SW);
    c->p_z[1] = k.take<half_t>(PR * SW);
    c->proj_rows = (int)PR;
    return OPUS_OK;
}

// The projector workspace holds c->proj_rows rows; larger inputs (the batched stage of the two-stage pipeline, SURVEY 8f N3:
// whole dataset shards at M >= 512, where the switch-projector GEMMs are MFMA-bound) are processed in chunks of that size.
static int protein_projector_rows(opus_ctx *c, hipStream_t s, const float *d_pooled, int B, half_t *d_out) {
    const opus_config &g = c->cfg;
    const int De = g.enc_dim;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_ERR * sizeof(int32_t), s));
    if (!g.has_protein_projector) {
        // IdentityModule.protein_forward (opus_arch.py:70-80): the pooled embedding itself feeds the switch projector,
        // whose autocast Linear rounds it to fp16
        KL(KC_OTHER, 6.0 * B * De, launch_f2h(d_pooled, (int64_t)B * De, d_out, s));
        return OPUS_OK;
    }
    KL(KC_NORM, 6.0 * B * De, launch_l2norm(d_pooled, B, De, c->p_xn, s));
    return gemm(c, s, c->p_xn, De, c->proj_w, B, g.proj_dim, De, c->proj_b, EPI_NONE, nullptr, d_out, g.proj_dim, 0);
}

static int switch_projector_rows(opus_ctx *c, hipStream_t s, const half_t *in, int B, half_t *d_out) {
    const opus_config &g = c->cfg;
    const int SW = g.dec_dim * g.n_prot_tokens;
    int din = g.has_protein_projector ? g.proj_dim : g.enc_dim;
    for (int i = 0; i < g.switch_depth; ++i) {
        const bool last = i + 1 == g.switch_depth;
        half_t *o = last ? d_out : c->p_z[i & 1];
        // nn.GELU() sits between the Linear layers (protein_mlp/builder.py:21-24): fused as the epilogue
        OPC(gemm(c, s, in, din, c->sw_w[i], B, SW, din, c->sw_b[i], last ? EPI_NONE : EPI_GELU, nullptr, o, SW, 0));
        in = o;
        din = SW;
    }
    return OPUS_OK;
}

extern "C" int opus_protein_projector(opus_ctx *c, const float *d_pooled, int32_t B, void *d_out, void *stream) {
    OPC(need_ready(c));
    if (!d_pooled || !d_out) return fail(OPUS_EBADARG, "protein_projector: null pointer");
    if (B < 1) return fail(OPUS_ESHAPE, "protein_projector: B=%d", B);
    const opus_config &g = c->cfg;
    const int64_t din = g.enc_dim, dout = g.has_protein_projector ? g.proj_dim : g.enc_dim;
    c->phase = PH_PROJECT;
    OPC(ensure_proj_rows(c, B));
    for (int r0 = 0; r0 < B; r0 += c->proj_rows) {
        const int n = B - r0 < c->proj_rows ? B - r0 : c->proj_rows;
        OPC(protein_projector_rows(c, (hipStream_t)stream, d_pooled + r0 * din, n, (half_t *)d_out + r0 * dout));
    }
    return OPUS_OK;
}

extern "C" int opus_switch_projector(opus_ctx *c, const void *d_in, int32_t B, void *d_out, void *stream) {
    OPC(need_ready(c));
    if (!d_in || !d_out) return fail(OPUS_EBADARG, "switch_projector: null pointer");
    if (B < 1) return fail(OPUS_ESHAPE, "switch_projector: B=%d", B);
    const opus_config &g = c->cfg;
    const int64_t din = g.has_protein_projector ? g.proj_dim : g.enc_dim, SW = (int64_t)g.dec_dim * g.n_prot_tokens;
    c->phase = PH_PROJECT;
    OPC(ensure_proj_rows(c, B));
    for (int r0 = 0; r0 < B; r0 += c->proj_rows) {
        const int n = B - r0 < c->proj_rows ? B - r0 : c->proj_rows;
        OPC(switch_projector_rows(c, (hipStream_t)stream, (const half_t *)d_in + r0 * din, n, (half_t *)d_out + r0 * SW));
    }
    return OPUS_OK;
}

extern "C" int opus_projector_forward(opus_ctx *c, const float *d_pooled, int32_t B, void *d_out, void *d_proj_out,
                                      void *stream) {
    OPC(need_ready(c));
    if (!d_pooled || !d_out) return fail(OPUS_EBADARG, "projector_forward: null pointer");
    if (B < 1) return fail(OPUS_ESHAPE, "projector_forward: B=%d", B);
    const opus_config &g = c->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int64_t din = g.enc_dim, dmid = g.has_protein_projector ? g.proj_dim : g.enc_dim, SW = (int64_t)g.dec_dim * g.n_prot_tokens;
    c->phase = PH_PROJECT;
    OPC(ensure_proj_rows(c, B));
    for (int r0 = 0; r0 < B; r0 += c->proj_rows) {
        const int n = B - r0 < c->proj_rows ? B - r0 : c->proj_rows;
        OPC(protein_projector_rows(c, s, d_pooled + r0 * din, n, c->p_y));
        if (d_proj_out)
            HIPC(hipMemcpyAsync((half_t *)d_proj_out + r0 * dmid, c->p_y, (size_t)n * dmid * sizeof(half_t), hipMemcpyDeviceToDevice, s));
        OPC(switch_projector_rows(c, s, c->p_y, n, (half_t *)d_out + r0 * SW));
    }
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ splice
extern "C" int opus_splice_pad(opus_ctx *c, const int64_t *d_ids, const uint8_t *d_mask, int32_t B, int32_t Tt,
                               const void *d_prot, int32_t n_prot, int32_t inference_mode, int32_t max_length,
                               void *d_embeds, uint8_t *d_mask_out, int32_t *d_pos_out, int32_t *T_out, void *stream) {
    OPC(need_ready(c));
    if (!d_ids || !d_prot || !d_embeds || !d_mask_out || !d_pos_out || !T_out) return fail(OPUS_EBADARG, "splice_pad: null pointer");
    const opus_config &g = c->cfg;
    if (B < 1 || B > g.max_batch || Tt < 1) return fail(OPUS_ESHAPE, "splice_pad: B=%d T_text=%d out of range", B, Tt);
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_SPLICE;
    KL(KC_OTHER, 9.0 * B * Tt, launch_splice_plan(d_ids, d_mask, B, Tt, g.n_prot_tokens, max_length, g.dec_vocab, c->d_plan, s));
    int32_t tail[3];
    HIPC(hipMemcpyAsync(tail, c->d_plan + 4 * B, sizeof(tail), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (tail[2]) return fail(OPUS_EBADARG, "splice_pad: token id outside [0, vocab) (and not -200)");
    if (tail[1] > n_prot) return fail(OPUS_ESHAPE, "splice_pad: rows consume %d protein blocks, %d supplied", tail[1], n_prot);
    if (tail[0] > g.max_prompt) return fail(OPUS_ESHAPE, "splice_pad: spliced length %d exceeds max_prompt=%d", tail[0], g.max_prompt);
    if (tail[0] < 1) return fail(OPUS_ESHAPE, "splice_pad: every row is empty");
    *T_out = tail[0];
    KL(KC_OTHER, 2.0 * B * tail[0] * g.dec_dim * 2,
       launch_splice_fill(d_ids, d_mask, B, Tt, (const half_t *)d_prot, g.n_prot_tokens, g.dec_dim, g.dec_vocab, c->dec_emb,
                          c->d_plan, tail[0], inference_mode ? 1 : 0, (half_t *)d_embeds, d_mask_out, d_pos_out, s));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ decoder
static int lm_head(opus_ctx *c, hipStream_t s, ResidShadow &sh, int B, float *out = nullptr) {
    const opus_config &g = c->cfg;   // final RMSNorm (folded weight) fused into the lm_head GEMM
    return gemm_norm(c, s, sh, c->d_xl, g.dec_rms_eps, c->d_xln, c->lm_head, B, g.dec_vocab, g.dec_dim, EPI_NONE, out ? out : c->d_logits,
                     g.dec_vocab, 1);
}

// End of a fanned-out prefill (nret > 1): the lm_head left the B prompts' last-position logits in d_probs (free until the sampling
// head runs); one launch replicates them into d_logits rows b nret + j and kstart[b] into kstart[b nret + j].  The K / V cache rows
// were replicated by the append itself (launch_dec_rope_cache's nret).
static int fanout_rows(opus_ctx *c, hipStream_t s, int B, int nret) {
    const opus_config &g = c->cfg;
    KL(KC_OTHER, 4.0 * (B + B * nret) * g.dec_vocab, launch_row_fanout(c->d_probs, c->d_logits, g.dec_vocab, B, nret, c->d_kstart, s));
    return OPUS_OK;
}


// d_step = {step counter = 0, T0 = prompt length}: the decode step's kernels read BOTH from the device (a captured step is
// then independent of the prompt length; through the kernel arguments, so the launch is stream-ordered and needs no host buffer)
static int reset_step(opus_ctx *c, hipStream_t s, int T0, int step = 0) {
    const int32_t v[2] = {step, T0};
    HIPC(launch_upload_i32(v, 2, c->d_step, s));
    return OPUS_OK;
}

// End of a prefill that keeps the last position only: the rows' last residual into d_xl (unless the last-layer tail left it there),
// the family's lm_head (`head(out)`; nret > 1: into d_probs, fanned out from there), the step words and the decode state.
template <class Head>
static int finish_prefill(opus_ctx *c, hipStream_t s, int B, int T, int nret, bool have_last, Head head) {
    const int H = c->cfg.dec_dim;
    if (!have_last) KL(KC_OTHER, 8.0 * B * H, launch_take_last(c->d_x, B, T, H, c->d_xl, s));
    OPC(head(nret > 1 ? c->d_probs : nullptr));
    if (nret > 1) OPC(fanout_rows(c, s, B, nret));
    OPC(reset_step(c, s, T));
    c->cur_B = B * nret;
    c->cur_T = T;
    c->prefilled = true;
    return OPUS_OK;
}

// decode-step attention of layer l over the projection output in d_qkv (rows of the last prefill, T prompt positions)
// (slab_ks > 0: the QKV GEMM left slab_ks raw k-part slabs in the GEMM workspace and the sums of squares of its input rows in
// d_ssq, sh.ssq_nblk blocks per row: summed, scaled and biased by the attention kernel itself)
static int attn_decode(opus_ctx *c, hipStream_t s, const ResidShadow &sh, int l, int B, int T, int slab_ks = 0, const float *bias = nullptr,
                       int out_tiled = 0) {
    const opus_config &g = c->cfg;
    AttnDecodeParams a;
    a.qkv = c->d_qkv; a.slabs = nullptr; a.ks = 0; a.slab_stride = 0; a.row_ssq = nullptr; a.row_nblk = 0; a.eps = 0.f; a.K = 0;
    a.bias = nullptr;
    if (slab_ks > 0) {
        const int64_t QKVd = (int64_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim;
        a.qkv = nullptr; a.slabs = c->gemm_ws; a.ks = slab_ks; a.slab_stride = (int64_t)B * QKVd;
        a.row_ssq = c->d_ssq; a.row_nblk = sh.ssq_nblk; a.eps = g.dec_rms_eps; a.K = g.dec_dim; a.bias = bias;
    }
    a.cs_row = c->cs_row; a.kstart = c->d_kstart; a.step = c->d_step; a.T0 = -1; a.nh = g.dec_heads; a.nkv = g.dec_kv_heads;   // (T0 < 0: d_step[1])
    a.kc = c->kc + l * c->cache_sl; a.vc = c->vc + l * c->cache_sl; a.cache_sb = c->cache_sb; a.cache_sh = c->cache_sh;
    a.ctx_cap = g.max_prompt + g.max_new_tokens; a.scale = 1.0f / sqrtf((float)g.dec_head_dim); a.out = c->d_ctx;
    a.out_tiled = out_tiled;
    // algorithmic bytes: the rows' K / V history once (+ the new token's q, k, v and the output)
    const double bytes = 4.0 * B * g.dec_kv_heads * g.dec_head_dim * (T + 1) + 2.0 * B * (2.0 * g.dec_heads + 2.0 * g.dec_kv_heads) * g.dec_head_dim;
    KL(KC_ATTN_DECODE, bytes, launch_attn_decode(a, B, g.dec_head_dim, s));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ OPT / Galactica decoder
// transformers OPTDecoder with do_layer_norm_before (reference wrapper language_model/opus_opt.py:18-40):
//   x = inputs_embeds + pos;  per layer  x += Wo attn(LN1 x) + bo;  x += W2 gelu(W1 LN2 x + b1) + b2;  logits = lm_head LNf x.
// No rotary: the (cos, sin) table holds (1, 0), so the fused rotate-and-cache kernels only append to the KV cache; the
// query scale head_dim^-0.5 is applied to the scores in fp32.
static int attn_prefix(opus_ctx *c, hipStream_t s, const ContRows &cr, int l, int M) {
    const opus_config &g = c->cfg;
    AttnPrefixParams a = cr.attn;
    a.kc = cr.snap_k ? cr.snap_k + l * cr.snap_sl : c->kc + l * c->cache_sl;
    a.vc = cr.snap_v ? cr.snap_v + l * cr.snap_sl : c->vc + l * c->cache_sl;
    const int QKV = (g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim, QD = g.dec_heads * g.dec_head_dim;
    // algorithmic bytes: the rows' projections + output, and every (prefix row, kv head)'s visible cache slots once
    KLF(KC_ATTN_PREFILL, 2.0 * M * (QKV + QD) + 4.0 * cr.nblocks * g.dec_kv_heads * g.dec_head_dim * a.Tp,
        4.0 * M * (double)QD * (a.Tp + a.n), launch_attn_prefix(a, cr.nblocks, s));
    return OPUS_OK;
}

// prefill attention of layer l over the B T projection rows in d_qkv: rotary + append to the KV cache (nret copies of every row) +
// causal attention; continuation rows (cont): rotary at their own positions, no cache write, attention behind the cached prefix
static int attn_prefill(opus_ctx *c, hipStream_t s, int l, int B, int T, const ContRows *cont, int nret) {
    const opus_config &g = c->cfg;
    const int nh = g.dec_heads, nkv = g.dec_kv_heads, hd = g.dec_head_dim, QKV = (nh + 2 * nkv) * hd, QD = nh * hd, M = B * T;
    if (cont) {
        KL(KC_OTHER, 4.0 * M * QKV, launch_dec_rope_cache(c->d_qkv, c->cs_dec, cont->nkst, B, T, nh, nkv, hd, nullptr, nullptr, 0, 0, s));
        if (cont->app_lens)
            KL(KC_OTHER, 8.0 * M * nkv * hd, launch_kv_append(c->d_qkv, cont->app_lens, B, T, nh, nkv, hd, cont->attn.Tp, c->kc + l * c->cache_sl,
                                                              c->vc + l * c->cache_sl, c->cache_sb, c->cache_sh, s));
        return attn_prefix(c, s, *cont, l, M);
    }
    KL(KC_OTHER, 4.0 * M * QKV,
       launch_dec_rope_cache(c->d_qkv, c->cs_dec, c->d_kstart, B, T, nh, nkv, hd, c->kc + l * c->cache_sl,
                             c->vc + l * c->cache_sl, c->cache_sb, c->cache_sh, s, nret));
    AttnParams a;
    a.Q = c->d_qkv; a.K = c->d_qkv + QD; a.V = c->d_qkv + QD + nkv * hd;
    a.q_sb = a.k_sb = a.v_sb = (int64_t)T * QKV;
    a.q_st = a.k_st = a.v_st = QKV;
    a.O = c->d_ctx; a.o_sb = (int64_t)T * QD; a.o_st = QD;
    a.kstart = c->d_kstart; a.kend = nullptr;
    a.B = B; a.T = T; a.heads = nh; a.group = nh / nkv; a.head_dim = hd; a.causal = 1;
    a.scale = 1.0f / sqrtf((float)hd);
    KLF(KC_ATTN_PREFILL, 2.0 * M * (QKV + QD), 2.0 * B * (double)T * T * QD, launch_attn_prefill(a, s));
    return OPUS_OK;
}

static int opt_layer(opus_ctx *c, hipStream_t s, const DecLayer &L, int l, float *x, half_t *xn, int M, int B, int T, bool decode,
                     const ContRows *cont = nullptr, int nret = 1) {
    const opus_config &g = c->cfg;
    const int H = g.dec_dim, F = g.dec_ffn;
    const int QKV = (g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim, QD = g.dec_heads * g.dec_head_dim;
    KL(KC_NORM, 6.0 * M * H, launch_layernorm(x, L.ln1w, L.ln1b, g.dec_rms_eps, M, H, xn, nullptr, s));
    OPC(gemm(c, s, xn, H, L.wqkv, M, QKV, H, L.bqkv, EPI_NONE, nullptr, c->d_qkv, QKV, 0));
    if (decode) OPC(attn_decode(c, s, ResidShadow(), l, B, T));
    else OPC(attn_prefill(c, s, l, B, T, cont, nret));
    OPC(gemm(c, s, c->d_ctx, QD, L.wo, M, H, QD, L.bo, EPI_NONE, x, x, H, 1));
    KL(KC_NORM, 6.0 * M * H, launch_layernorm(x, L.ln2w, L.ln2b, g.dec_rms_eps, M, H, xn, nullptr, s));
    if (g.dec_act == 0) {
        OPC(gemm(c, s, xn, H, L.w1, M, F, H, L.b1, EPI_GELU, nullptr, c->d_act, F, 0));
    } else {      // ReLU (facebook/opt-*): on the stored fp16 projection, as HF applies it to fc1's fp16 output
        OPC(gemm(c, s, xn, H, L.w1, M, F, H, L.b1, EPI_NONE, nullptr, c->d_act, F, 0));
        KL(KC_OTHER, 4.0 * M * F, launch_relu_h(c->d_act, (int64_t)M * F, s));
    }
    OPC(gemm(c, s, c->d_act, F, L.w2, M, H, F, L.b2, EPI_NONE, x, x, H, 1));
    return OPUS_OK;
}

static int lm_head_opt(opus_ctx *c, hipStream_t s, int B, float *out = nullptr) {
    const opus_config &g = c->cfg;
    KL(KC_NORM, 6.0 * B * g.dec_dim, launch_layernorm(c->d_xl, c->dec_lnfw, c->dec_lnfb, g.dec_rms_eps, B, g.dec_dim, c->d_xln, nullptr, s));
    return gemm(c, s, c->d_xln, g.dec_dim, c->lm_head, B, g.dec_vocab, g.dec_dim, nullptr, EPI_NONE, nullptr, out ? out : c->d_logits,
                g.dec_vocab, 1);
}

static int prefill_opt(opus_ctx *c, hipStream_t s, const half_t *embeds, const uint8_t *mask, int B, int T, bool all_rows,
                       const ContRows *cont, int nret) {
    const opus_config &g = c->cfg;
    const int H = g.dec_dim, M = B * T;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_ERR * sizeof(int32_t), s));
    if (!cont) KL(KC_OTHER, 1.0 * M, launch_mask_to_kstart(mask, B, T, c->d_kstart, s));
    KL(KC_OTHER, 6.0 * M * H, launch_h2f(embeds, c->d_x, (int64_t)M * H, s));
    KL(KC_OTHER, 10.0 * M * H, launch_add_pos(c->d_x, c->dec_pos, cont ? cont->nkst : c->d_kstart, nullptr, 0, B, T, H, g.dec_max_pos + 1, s));
    for (int l = 0; l < g.dec_layers; ++l) OPC(opt_layer(c, s, c->dec[l], l, c->d_x, c->d_xn, M, B, T, false, cont, nret));
    if (all_rows) return OPUS_OK;
    return finish_prefill(c, s, B, T, nret, false, [&](float *out) { return lm_head_opt(c, s, B, out); });
}

// the embedded new tokens are already in d_xl (decode_step)
static int decode_step_opt(opus_ctx *c, hipStream_t s) {
    const opus_config &g = c->cfg;
    const int B = c->cur_B, T = c->cur_T, H = g.dec_dim;
    KL(KC_OTHER, 10.0 * B * H, launch_add_pos(c->d_xl, c->dec_pos, c->d_kstart, c->d_step, -1, B, 1, H, g.dec_max_pos + 1, s));   // (t0 < 0: d_step[1])
    for (int l = 0; l < g.dec_layers; ++l) OPC(opt_layer(c, s, c->dec[l], l, c->d_xl, c->d_xln, B, B, T, true));
    OPC(lm_head_opt(c, s, B));
    KL(KC_OTHER, 8.0, launch_step_advance(c->d_step, s));
    return OPUS_OK;
}

// all_rows: every position of every row runs through the last layer too, and the final residual stream of all B T rows is left in
// d_x for opus_llama_forward; no lm_head, and the context is left without a prefill (decode_step fails until the next one).
// cont: the B rows are continuations behind the cached prefix (ContRows; implies all_rows, mask unused): kstart, the step word
// and the decode state are left as they are, and so is the KV cache unless ContRows::app_lens is set (opus_llama_prefill_behind:
// the rows' K / V are appended behind their prefix; the caller then sets kstart, the step word and the decode state itself).
// nret > 1 (never with all_rows or cont): the fanned-out prefill - the B prompts run once, and the context is left as after a prefill of
// every prompt repeated nret times (cur_B = B nret; cache rows, kstart and the last logits of prompt b in rows b nret + j).
static int prefill(opus_ctx *c, hipStream_t s, const half_t *embeds, const uint8_t *mask, int B, int T, bool all_rows = false,
                   const ContRows *cont = nullptr, int nret = 1) {
    c->phase = cont && !cont->app_lens ? PH_SCORE : PH_PREFILL;      // (rows that append to the cache: opus_llama_prefill_behind)
    if (cont && cont->w8) c->phase = PH_DECODE;                      // (a verify pass of the decode loop)
    if (cont) {
        all_rows = true;
    } else {
        new_epoch(c);
        if (all_rows) {
            c->prefilled = false;
            c->cur_B = 0;
        }
    }
    if (c->cfg.dec_arch == 1) return prefill_opt(c, s, embeds, mask, B, T, all_rows, cont, nret);
    const opus_config &g = c->cfg;
    const int H = g.dec_dim, F = g.dec_ffn, nh = g.dec_heads, nkv = g.dec_kv_heads, hd = g.dec_head_dim;
    const int QKV = (nh + 2 * nkv) * hd, QD = nh * hd;
    const int M = B * T;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_ERR * sizeof(int32_t), s));       // hand-off words start from zero on every call
    if (!cont) KL(KC_OTHER, 1.0 * M, launch_mask_to_kstart(mask, B, T, c->d_kstart, s));
    KL(KC_OTHER, 6.0 * M * H, launch_h2f(embeds, c->d_x, (int64_t)M * H, s));
    // RMSNorm fused around the big tiled GEMM, as the encoder's LayerNorm (GemmParams::ln_* with mu = 0): the wo / down epilogue
    // leaves fp16(x) + per-slab sums of squares, the consuming projection scales its rows by rstd in its epilogue
    static const bool no_ln_env = getenv("OPUS_NO_LN_FUSION") != nullptr;      // A/B aid (also the knob of the same name)
    const bool no_ln_fusion = no_ln_env || g_knobs.no_ln_fusion;
    const bool qkv_pp = !no_ln_fusion && (H & 255) == 0 && (QKV & 255) == 0 && gemm_goes_pp(M, QKV);
    const bool gu_pp = !no_ln_fusion && (H & 255) == 0 && (F & 127) == 0 && gemm_goes_pp(M, 2 * F);
    bool have_stat = false, last_rows_done = false;
    auto finalize = [&]() -> int {
        KL(KC_NORM, 8.0 * M * (H / 64) + 8.0 * M, launch_ln_finalize(c->d_part, M, H / 64, H, g.dec_rms_eps, 1, c->d_stat, s));
        return OPUS_OK;
    };
    ResidShadow sh;
    GemmGot got;
    const bool w8 = cont && cont->w8;                                // (false: every ask below is what it was)
    auto ask8 = [&](GemmAsk a, const QuantW &q) { return w8 ? a.quant(q) : a; };
    for (int l = 0; l < g.dec_layers; ++l) {
        const DecLayer &L = c->dec[l];
        if (have_stat && qkv_pp) {
            OPC(gemm(c, s, c->d_xn, H, L.wqkv, M, QKV, H, L.bqkv, EPI_NONE, nullptr, c->d_qkv, QKV, 0, GemmAsk().ln_consume(c->d_stat, nullptr)));
        } else {
            OPC(gemm_norm(c, s, sh, c->d_x, g.dec_rms_eps, c->d_xn, L.wqkv, M, QKV, H, EPI_NONE, c->d_qkv, QKV, 0, L.bqkv,
                          ask8(GemmAsk(), L.wq_qkv)));
        }
        OPC(attn_prefill(c, s, l, B, T, cont, nret));
        if (l + 1 == g.dec_layers && T > 1 && !all_rows && !g_knobs.misc[7]) {
            // Last layer: its K / V are in the cache for every position, but behind the attention only the LAST position of a row
            // is ever used (lm_head reads that row alone, opus_arch.py -> HF generate keeps the last logits): wo, gate/up and
            // down run on B rows with the decode step's kernels instead of on B T rows (Llama-3-8B, 64 x 96: ~1.85 ms of tiled
            // GEMMs -> ~0.1 ms; same values for the rows that are kept).  Knob misc7 = 1: all rows, as every other layer.
            half_t *ctx_last = c->d_qkv;                              // (the projections are consumed: the buffer is free)
            KL(KC_OTHER, 4.0 * B * QD, launch_take_last(reinterpret_cast<const float *>(c->d_ctx), B, T, QD / 2, reinterpret_cast<float *>(ctx_last), s));
            KL(KC_OTHER, 8.0 * B * H, launch_take_last(c->d_x, B, T, H, c->d_xl, s));
            const GemmAsk copy_xl = GemmAsk().copy16(fuse_rows() && B <= 96 ? c->d_xln : nullptr);
            OPC(gemm(c, s, ctx_last, QD, L.wo, B, H, QD, nullptr, EPI_NONE, c->d_xl, c->d_xl, H, 1, copy_xl, &got));
            sh.produced(c->d_xl, got);
            OPC(gemm_norm(c, s, sh, c->d_xl, g.dec_rms_eps, c->d_xln, L.wgu, B, 2 * F, H, EPI_SILU_GU16, c->d_act, F, 0));
            OPC(gemm(c, s, c->d_act, F, L.wd, B, H, F, nullptr, EPI_NONE, c->d_xl, c->d_xl, H, 1, copy_xl, &got));
            sh.produced(c->d_xl, got);
            last_rows_done = true;
            break;
        }
        GemmAsk wo;
        if (gu_pp) wo.ln_produce(c->d_part, c->d_xn);
        else if (fuse_rows() && M <= 96) wo.copy16(c->d_xn);      // (d_ssq holds 128 rows)
        OPC(gemm(c, s, c->d_ctx, QD, L.wo, M, H, QD, nullptr, EPI_NONE, c->d_x, c->d_x, H, 1, ask8(wo, L.wq_o), &got));
        sh.produced(c->d_x, got);
        have_stat = got.ln_done != 0;
        if (have_stat) {
            OPC(finalize());
            OPC(gemm(c, s, c->d_xn, H, L.wgu, M, 2 * F, H, nullptr, EPI_SILU_GU16, nullptr, c->d_act, F, 0, GemmAsk().ln_consume(c->d_stat, nullptr)));
        } else {
            OPC(gemm_norm(c, s, sh, c->d_x, g.dec_rms_eps, c->d_xn, L.wgu, M, 2 * F, H, EPI_SILU_GU16, c->d_act, F, 0, nullptr,
                          ask8(GemmAsk(), L.wq_gu)));
        }
        const bool next_pp = qkv_pp && l + 1 < g.dec_layers;
        OPC(gemm(c, s, c->d_act, F, L.wd, M, H, F, nullptr, EPI_NONE, c->d_x, c->d_x, H, 1, ask8(GemmAsk().ln_produce(next_pp ? c->d_part : nullptr, c->d_xn), L.wq_d), &got));
        have_stat = got.ln_done != 0;
        if (have_stat) OPC(finalize());
    }
    if (all_rows) return OPUS_OK;
    return finish_prefill(c, s, B, T, nret, last_rows_done, [&](float *out) { return lm_head(c, s, sh, B, out); });
}

// One decode step for the token ids in d_tok (device): embeds them, runs the stack at slot T + *step,
// leaves logits in c->d_logits and advances *step.
static int decode_step(opus_ctx *c, hipStream_t s, const int32_t *d_tok) {
    c->phase = PH_DECODE;
    const opus_config &g = c->cfg;
    const int B = c->cur_B, T = c->cur_T;
    const int H = g.dec_dim, F = g.dec_ffn, nh = g.dec_heads, nkv = g.dec_kv_heads, hd = g.dec_head_dim;
    const int QKV = (nh + 2 * nkv) * hd, QD = nh * hd;
    const int ctx_cap = g.max_prompt + g.max_new_tokens;
    // batched Llama / Qwen2 step: the embedding kernel also leaves fp16(x) and its per-block sums of squares, so that the first
    // layer's QKV GEMM can take the row-scale RMSNorm form like every later one (whose producer is the previous down GEMM)
    const bool rowscale = g.dec_arch == 0 && fuse_rows() && B > SKINNY_MAX_M && B <= MID_MAX_M && (H & 255) == 0;
    // Fragment-ordered fp16 activations for the GEMMs that gemm_stream_kernel will take (gemm_stream.hip "Activation layout"):
    // the producer of each such matrix is told to write that layout - fp16(x) for the QKV projection (embedding kernel for
    // layer 0, the down projection's epilogue / reduce afterwards) and the attention output for the wo projection.
    const bool qkv_tiled = rowscale && gemm_stream_would(B, QKV, H, 1, 1, 1, c->gemm_ws_bytes);
    const bool wo_tiled = rowscale && gemm_stream_would(B, H, QD, 0, 1, 0, c->gemm_ws_bytes);
    const bool down_tiled = rowscale && (F & 63) == 0 && gemm_stream_would(B, H, F, 0, 1, 0, c->gemm_ws_bytes);
    KL(KC_OTHER, 6.0 * B * H, launch_embed_tokens(d_tok, c->dec_emb, B, H, g.dec_vocab, c->d_xl, rowscale ? c->d_xln : nullptr,
                                                  rowscale ? c->d_ssq : nullptr, qkv_tiled ? 1 : 0, c->cs_dec, c->d_kstart, c->d_step, -1,
                                                  hd / 2, c->cs_row, c->d_cnt, HANDOFF_ERR, s));     // (+ zeroes the hand-off words; T0 < 0: d_step[1])
    if (g.dec_arch == 1) return decode_step_opt(c, s);
    ResidShadow sh;                      // (the embedding kernel is the first producer)
    if (rowscale) { sh.xh_src = c->d_xl; sh.ssq_nblk = H >> 8; sh.xln_tiled = qkv_tiled; }
    GemmGot got;
    half_t *const copy_xl = fuse_rows() && B <= 96 ? c->d_xln : nullptr;   // fp16(x) + sums of squares, asked of wo and down
    for (int l = 0; l < g.dec_layers; ++l) {
        const DecLayer &L = c->dec[l];
        if (rowscale && sh.xh_src == c->d_xl) {
            // x is available as fp16 + sums of squares (from the embedding or the previous layer's down GEMM): the QKV
            // projection streams its weights through the wide kernel with k-parts and leaves the raw slabs; the attention
            // kernel sums them, applies the RMSNorm row scale and the bias on the fly - no norm launch, no reduce launch
            sh.xh_src = nullptr;
            OPC(gemm(c, s, c->d_xln, H, L.wqkv, B, QKV, H, L.bqkv, EPI_NONE, nullptr, c->d_qkv, QKV, 0,
                     GemmAsk().slabs().scale_rows(g.dec_rms_eps, sh.ssq_nblk).tiled_a(sh.xln_tiled).quant(L.wq_qkv), &got));
            OPC(attn_decode(c, s, sh, l, B, T, got.ks > 1 ? got.ks : 0, L.bqkv, wo_tiled ? 1 : 0));
        } else {
            OPC(gemm_norm(c, s, sh, c->d_xl, g.dec_rms_eps, c->d_xln, L.wqkv, B, QKV, H, EPI_NONE, c->d_qkv, QKV, 0, L.bqkv,
                          GemmAsk().quant(L.wq_qkv)));
            OPC(attn_decode(c, s, sh, l, B, T, 0, nullptr, wo_tiled ? 1 : 0));
        }
        // (the copy row-major: the gate/up kernel stages it by LDS-DMA)
        OPC(gemm(c, s, c->d_ctx, QD, L.wo, B, H, QD, nullptr, EPI_NONE, c->d_xl, c->d_xl, H, 1, GemmAsk().copy16(copy_xl).tiled_a(wo_tiled).quant(L.wq_o), &got));
        sh.produced(c->d_xl, got);
        // the gate / up kernel writes silu(g) u in fragment order when the down projection will read it that way (only the wide
        // kernel - the row-scale form of gemm_norm - writes that layout)
        const bool act_tiled = down_tiled && sh.xh_src == c->d_xl && gemm_goes_wide(B, 2 * F);
        OPC(gemm_norm(c, s, sh, c->d_xl, g.dec_rms_eps, c->d_xln, L.wgu, B, 2 * F, H, EPI_SILU_GU16, c->d_act, F, 0, nullptr, GemmAsk().tiled_c(act_tiled).quant(L.wq_gu)));
        const bool next_tiled = qkv_tiled && l + 1 < g.dec_layers;      // (the last layer's fp16(x) feeds lm_head: row-major)
        OPC(gemm(c, s, c->d_act, F, L.wd, B, H, F, nullptr, EPI_NONE, c->d_xl, c->d_xl, H, 1, GemmAsk().copy16(copy_xl, next_tiled).tiled_a(act_tiled).quant(L.wq_d), &got));
        sh.produced(c->d_xl, got, next_tiled);
    }
    OPC(lm_head(c, s, sh, B));
    KL(KC_OTHER, 8.0, launch_step_advance(c->d_step, s));
    return OPUS_OK;
}

// Synchronises `s` and reports an in-launch hand-off that gave up waiting (GemmParams::combine_cnt[HANDOFF_ERR], set by a kernel
// whose bounded wait ran out: poisoned ticket words, a partner that never arrived).  The results of that call are not to be used.
static int handoff_check(opus_ctx *c, hipStream_t s) {
    int32_t err = 0;
    HIPC(hipMemcpyAsync(&err, c->d_cnt + HANDOFF_ERR, sizeof(err), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (!err) return OPUS_OK;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_WORDS * sizeof(int32_t), s));
    return fail(OPUS_EHIP, "an in-launch hand-off (split-K combine) gave up waiting for its partner: results of this call are invalid");
}

extern "C" int opus_check_error(opus_ctx *c, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    HIPC(hipSetDevice(c->device));
    return handoff_check(c, (hipStream_t)stream);
}

static int check_prefill_args(opus_ctx *c, const void *e, const uint8_t *m, int B, int T) {
    if (!e || !m) return fail(OPUS_EBADARG, "prefill: null pointer");
    if (B < 1 || B > c->cfg.max_batch || T < 1 || T > c->cfg.max_prompt)
        return fail(OPUS_ESHAPE, "prefill: B=%d T=%d exceed capacity (%d, %d)", B, T, c->cfg.max_batch, c->cfg.max_prompt);
    return OPUS_OK;
}

extern "C" int opus_llama_prefill(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                                  float *d_last_logits, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    hipStream_t s = (hipStream_t)stream;
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T));
    if (d_last_logits)
        HIPC(hipMemcpyAsync(d_last_logits, c->d_logits, (size_t)B * c->cfg.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

static int check_fanout(opus_ctx *c, int B, int nret, const char *who) {
    if (nret < 1) return fail(OPUS_EBADARG, "%s: nret=%d (at least 1)", who, nret);
    if ((int64_t)B * nret > c->cfg.max_batch)
        return fail(OPUS_ESHAPE, "%s: B x nret = %d x %d decoder rows, the context holds max_batch=%d", who, B, nret, c->cfg.max_batch);
    return OPUS_OK;
}

extern "C" int opus_llama_prefill_fanout(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t nret,
                                         float *d_last_logits, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    OPC(check_fanout(c, B, nret, "prefill_fanout"));
    hipStream_t s = (hipStream_t)stream;
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T, false, nullptr, nret));
    if (d_last_logits)
        HIPC(hipMemcpyAsync(d_last_logits, c->d_logits, (size_t)B * nret * c->cfg.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

extern "C" int opus_llama_decode_step(opus_ctx *c, const int32_t *d_tok, float *d_logits, void *stream) {
    OPC(need_ready(c));
    if (!c->prefilled) return fail(OPUS_ESTATE, "decode_step before prefill");
    if (!d_tok) return fail(OPUS_EBADARG, "decode_step: null pointer");
    hipStream_t s = (hipStream_t)stream;
    int32_t st = 0;
    HIPC(hipMemcpyAsync(&st, c->d_step, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (st >= c->cfg.max_new_tokens) return fail(OPUS_ESHAPE, "decode_step: KV cache is full (%d steps)", st);
    OPC(decode_step(c, s, d_tok));
    if (d_logits)
        HIPC(hipMemcpyAsync(d_logits, c->d_logits, (size_t)c->cur_B * c->cfg.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ teacher-forced scoring
// Logits slab of one loss-only chunk: at most this many bytes (well inside the 256 MiB Infinity Cache, so that the NLL kernel
// may find the GEMM's output there).
static constexpr int64_t SCORE_SLAB_BYTES = 128ll << 20;

// Rows per chunk of the score phase: all R, or (loss-only) as many as a logits slab holds - whole multiples of 64 from 64 up.
static int64_t score_chunk_cap(const opus_config &g, int64_t R, bool loss_only) {
    if (!loss_only) return R;
    const int64_t cap = SCORE_SLAB_BYTES / ((int64_t)g.dec_vocab * (int64_t)sizeof(half_t));
    return std::min(R, cap >= 64 ? cap & ~(int64_t)63 : std::max<int64_t>(cap, 1));
}
// caller scratch a chunk of n rows needs: the gathered fp32 rows (+ the logits slab when loss-only)
static int64_t score_chunk_bytes(const opus_config &g, int64_t n, bool loss_only) {
    return (int64_t)align_up((size_t)n * g.dec_dim * sizeof(float)) +
           (loss_only ? (int64_t)align_up((size_t)n * g.dec_vocab * sizeof(half_t)) : 0);
}
// the chunk the caller's scratch allows (a smaller scratch than opus_llama_forward_scratch_bytes asks for: smaller chunks)
static int64_t score_chunk_rows(const opus_config &g, int64_t R, bool loss_only, int64_t scratch_bytes) {
    int64_t n = score_chunk_cap(g, R, loss_only);
    while (n > 0 && score_chunk_bytes(g, n, loss_only) > scratch_bytes) n = n >= 128 ? (n / 2) & ~(int64_t)63 : n - 1;
    return n;
}

static int ensure_topk_mem(opus_ctx *c);

// final norm + lm_head over the n fp32 rows in X -> operand-dtype logits [n, V] (row stride V), then the NLL of every row
static int score_rows(opus_ctx *c, hipStream_t s, const float *X, int n, half_t *logits, const int32_t *targets, float *logprob,
                      float *lse) {
    const opus_config &g = c->cfg;
    const int H = g.dec_dim, V = g.dec_vocab;
    if (g.dec_arch == 1) {
        KL(KC_NORM, 6.0 * n * H, launch_layernorm(X, c->dec_lnfw, c->dec_lnfb, g.dec_rms_eps, n, H, c->d_xn, nullptr, s));
        OPC(gemm(c, s, c->d_xn, H, c->lm_head, n, V, H, nullptr, EPI_NONE, nullptr, logits, V, 0));
    } else {   // RMSNorm folded into lm_head: fused into the skinny / mid kernels, a weight-less norm into d_xn otherwise
        ResidShadow none;                // (gathered rows: no producer left a copy of them)
        OPC(gemm_norm(c, s, none, X, g.dec_rms_eps, c->d_xn, c->lm_head, n, V, H, EPI_NONE, logits, V, 0));
    }
    KL(KC_XENT, 2.0 * n * V + 12.0 * n, launch_xent(logits, V, n, V, targets, logprob, lse, s));
    return OPUS_OK;
}

extern "C" int opus_llama_forward(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                                  const int32_t *d_rows, int32_t R, const int32_t *d_targets, float *d_logprob, void *d_logits,
                                  void *d_scratch, int64_t scratch_bytes, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    if (R < 0 || (int64_t)R > (int64_t)B * T) return fail(OPUS_ESHAPE, "forward: R=%d rows of a %d x %d batch", R, B, T);
    if (R > 0 && (!d_rows || !d_targets || !d_logprob)) return fail(OPUS_EBADARG, "forward: null rows / targets / logprob");
    const opus_config &g = c->cfg;
    const bool loss_only = d_logits == nullptr;
    const int64_t chunk = R > 0 ? score_chunk_rows(g, R, loss_only, d_scratch ? scratch_bytes : 0) : 0;
    if (R > 0 && chunk < 1)
        return fail(OPUS_EBADARG, "forward: scratch of %lld bytes holds no row (opus_llama_forward_scratch_bytes)", (long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (c->top_k > 0 && R > 0) {             // the chunk's log-sum-exp rows (grown on use; the stream is idle between forward calls)
        OPC(ensure_topk_mem(c));
        if (chunk > c->fwd_lse_cap) {
            HIPC(hipStreamSynchronize(s));
            if (c->fwd_lse) (void)hipFree(c->fwd_lse);
            c->fwd_lse = nullptr; c->fwd_lse_cap = 0;
            HIPC(hipMalloc((void **)&c->fwd_lse, align_up((size_t)chunk * sizeof(float))));
            c->fwd_lse_cap = chunk;
        }
    }
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T, true));
    c->phase = PH_SCORE;
    const int H = g.dec_dim, V = g.dec_vocab;
    float *rows_f = reinterpret_cast<float *>(d_scratch);
    half_t *slab = loss_only ? reinterpret_cast<half_t *>((char *)d_scratch + align_up((size_t)chunk * H * sizeof(float))) : nullptr;
    for (int64_t r0 = 0; r0 < R; r0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, R - r0);
        KL(KC_OTHER, 8.0 * n * H + 4.0 * n, launch_gather_rows(c->d_x, d_rows + r0, n, (int64_t)B * T, H, rows_f, s));
        half_t *out = loss_only ? slab : reinterpret_cast<half_t *>(d_logits) + r0 * V;
        OPC(score_rows(c, s, rows_f, n, out, d_targets + r0, d_logprob + r0, c->top_k > 0 ? c->fwd_lse : nullptr));
        // opus_set_gen_top_logprobs: the k likeliest ids of every scored row, [R, k], from the chunk's 16-bit logits and xent's lse
        for (int q0 = 0; c->top_k > 0 && q0 < n; q0 += c->topk_rows()) {
            const int m = std::min(n - q0, c->topk_rows());
            TopkArgs ta;
            ta.cand = c->d_tcand; ta.lse = c->fwd_lse + q0; ta.k = c->top_k;
            ta.ids = c->top_ids + (r0 + q0) * c->top_k; ta.lp = c->top_lp + (r0 + q0) * c->top_k;
            KL(KC_TOPK, 2.0 * m * V, launch_topk_h16(out + (int64_t)q0 * V, V, m, V, ta, s));
        }
    }
    return OPUS_OK;
}

extern "C" int64_t opus_llama_forward_scratch_bytes(const opus_config *cfg, int32_t R, int32_t with_logits) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    if (R < 0) {
        fail(OPUS_ESHAPE, "forward_scratch_bytes: R=%d", R);
        return -1;
    }
    return R == 0 ? 0 : score_chunk_bytes(*cfg, score_chunk_cap(*cfg, R, !with_logits), !with_logits);
}

extern "C" int opus_debug_xent(opus_ctx *c, const void *d_logits, int32_t R, int32_t V, const int32_t *d_targets, float *d_logprob,
                               float *d_lse, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!d_logits || !d_targets || !d_logprob) return fail(OPUS_EBADARG, "debug_xent: null pointer");
    if (R < 0 || V < 1) return fail(OPUS_ESHAPE, "debug_xent: R=%d V=%d", R, V);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_SCORE;
    KL(KC_XENT, 2.0 * R * V + 12.0 * R, launch_xent((const half_t *)d_logits, V, R, V, d_targets, d_logprob, d_lse, s));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ shared-prefix scoring
// opus_llama_prefix = a prefill that also hands out the final residual rows of every row's last position and the cache epoch;
// opus_llama_score_continuations runs continuation rows behind that cached prefix (prefill()'s layer loop with ContRows) and
// scores them: the first token of a continuation from the prefix's last row, token j >= 1 from continuation position j - 1.

// rows the decoder activation buffers hold (carve's Md)
static int64_t dec_rows_cap(const opus_config &g) {
    const int64_t B16 = ((int64_t)g.max_batch + 15) & ~(int64_t)15;
    return std::max<int64_t>((int64_t)g.max_batch * g.max_prompt, B16);
}
// continuation rows per pass of the layer loop: as many as the prefill's activation buffers hold positions (not max_batch rows)
static int64_t prefix_group_rows(const opus_config &g, int64_t R, int n) { return std::min<int64_t>(R, dec_rows_cap(g) / n); }
// int32 table words of one pass of Rg rows: row offsets per prefix row, row list, position bases, workgroup table, gather index
static int64_t prefix_table_words(const opus_config &g, int64_t Rg, int n) {
    const int G = g.dec_heads / g.dec_kv_heads;
    return (int64_t)g.max_batch + 1 + 2 * Rg + 2 * (int64_t)attn_prefix_max_blocks((int)Rg, g.max_batch, G, n) + Rg * n;
}
static int64_t prefix_scratch_bytes(const opus_config &g, int64_t R, int n) {
    const int64_t Rg = prefix_group_rows(g, R, n);
    return (int64_t)align_up((size_t)prefix_table_words(g, Rg, n) * sizeof(int32_t)) +
           score_chunk_bytes(g, score_chunk_cap(g, Rg * n, true), true);
}

// host tables of one pass: rows src[0 .. Rg) (local row ids) grouped by prefix row, in the layout AttnPrefixParams reads
struct PrefixTables {
    std::vector<int32_t> w;
    int off = 0, list = 0, nkst = 0, blocks = 0, gidx = 0, nblocks = 0;
};
static void build_prefix_tables(const opus_config &g, const std::vector<int32_t> &kst, int Tp, const int32_t *src, int Rg, int n,
                                PrefixTables &t) {
    const int P = (int)kst.size(), G = g.dec_heads / g.dec_kv_heads;
    t.off = 0;
    t.list = P + 1;
    t.nkst = t.list + Rg;
    t.blocks = t.nkst + Rg;
    t.w.assign((size_t)t.blocks, 0);
    for (int r = 0; r < Rg; ++r) ++t.w[t.off + src[r] + 1];
    for (int p = 0; p < P; ++p) t.w[t.off + p + 1] += t.w[t.off + p];
    std::vector<int32_t> fill(t.w.begin() + t.off, t.w.begin() + t.off + P);
    for (int r = 0; r < Rg; ++r) {
        t.w[t.list + fill[src[r]]++] = r;
        t.w[t.nkst + r] = kst[src[r]] - Tp;               // rotary / learned position of new position j: Tp - kstart[p] + j
    }
    t.nblocks = attn_prefix_blocks(t.w.data() + t.off, P, G, n, nullptr);
    t.w.resize((size_t)t.blocks + 2 * t.nblocks);
    attn_prefix_blocks(t.w.data() + t.off, P, G, n, t.w.data() + t.blocks);
    t.gidx = (int)t.w.size();
}
// the kernel's parameters for the tables t uploaded at d_tbl (par, for the tree form, is set by the caller that has it)
static AttnPrefixParams prefix_params(const opus_ctx *c, const int32_t *d_tbl, const PrefixTables &t, int Tp, int n, const half_t *qkv,
                                      const half_t *kc, const half_t *vc, half_t *out) {
    const opus_config &g = c->cfg;
    AttnPrefixParams a;
    a.kc = kc; a.vc = vc; a.cache_sb = c->cache_sb; a.cache_sh = c->cache_sh; a.kstart = c->d_kstart; a.Tp = Tp;
    a.qkv = qkv; a.n = n; a.list = d_tbl + t.list; a.off = d_tbl + t.off; a.blocks = d_tbl + t.blocks; a.out = out;
    a.nh = g.dec_heads; a.nkv = g.dec_kv_heads; a.hd = g.dec_head_dim; a.scale = 1.0f / sqrtf((float)g.dec_head_dim);
    return a;
}
// is the prefix handle (P, epoch) of opus_llama_prefix still what this context's cache holds?
static int check_current_prefix(const opus_ctx *c, const char *who, int P, int64_t epoch) {
    if (!c->prefilled || epoch != c->epoch || (int)c->h_kstart.size() != c->cur_B || P != c->cur_B)
        return fail(OPUS_ESTATE, "%s: the prefix is not this context's current one (a later call prefilled or permuted the cache, or "
                                 "the handle belongs to another context)", who);
    return OPUS_OK;
}
// Where a pass behind a prefix finds it: the context's current prefill (snap == nullptr: the handle's P and epoch are checked) or
// a detached snapshot (opus_prefix_snap: no epoch - it never goes stale - and any context of the same configuration)
struct PrefixSrc {
    int P = 0, Tp = 0;
    std::vector<int32_t> kst;            // first visible slot of every prefix row (host)
    const opus_prefix_snap *snap = nullptr;
    // the pass reads the snapshot instead of the context's cache: same kernel, other base pointers and strides
    void apply(const opus_config &g, ContRows &cr) const {
        if (!snap) return;
        cr.snap_k = reinterpret_cast<const half_t *>(snap->d_k);
        cr.snap_v = reinterpret_cast<const half_t *>(snap->d_v);
        cr.attn.cache_sh = (int64_t)Tp * g.dec_head_dim;
        cr.attn.cache_sb = cr.attn.cache_sh * g.dec_kv_heads;
        cr.snap_sl = cr.attn.cache_sb * P;
        cr.attn.kstart = snap->d_kstart;
    }
};
static int resolve_prefix(const opus_ctx *c, const char *who, const opus_prefix_snap *snap, int P, int64_t epoch, PrefixSrc &ps) {
    ps.snap = snap;
    if (!snap) {
        OPC(check_current_prefix(c, who, P, epoch));
        ps.P = P;
        ps.Tp = c->cur_T;
        ps.kst = c->h_kstart;
        return OPUS_OK;
    }
    if (!snap->d_k || !snap->d_v || !snap->d_kstart || !snap->h_kstart) return fail(OPUS_EBADARG, "%s: null pointer in the prefix snapshot", who);
    if (snap->P < 1 || snap->P > c->cfg.max_batch || snap->Tp < 1 || snap->Tp > c->cfg.max_prompt)
        return fail(OPUS_ESHAPE, "%s: a snapshot of %d rows x %d slots, the context holds max_batch=%d rows and max_prompt=%d slots", who,
                    snap->P, snap->Tp, c->cfg.max_batch, c->cfg.max_prompt);
    for (int p = 0; p < snap->P; ++p)
        if (snap->h_kstart[p] < 0 || snap->h_kstart[p] >= snap->Tp)
            return fail(OPUS_EBADARG, "%s: kstart[%d]=%d of the snapshot outside [0, %d)", who, p, snap->h_kstart[p], snap->Tp);
    ps.P = snap->P;
    ps.Tp = snap->Tp;
    ps.kst.assign(snap->h_kstart, snap->h_kstart + snap->P);
    return OPUS_OK;
}
// layer 0 of the KV cache <- a history d_k_hist / d_v_hist [rows, kv heads, L, hd] (slots 0 .. L - 1) and kstart <- d_kstart [rows]
// (the kernel-level debug entries)
static int seed_cache(opus_ctx *c, hipStream_t s, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart, int rows, int L) {
    const int nkv = c->cfg.dec_kv_heads;
    const size_t pitch = (size_t)c->cache_sh * sizeof(half_t), roww = (size_t)L * c->cfg.dec_head_dim * sizeof(half_t);
    HIPC(hipMemcpy2DAsync(c->kc, pitch, d_k_hist, roww, roww, (size_t)rows * nkv, hipMemcpyDeviceToDevice, s));
    HIPC(hipMemcpy2DAsync(c->vc, pitch, d_v_hist, roww, roww, (size_t)rows * nkv, hipMemcpyDeviceToDevice, s));
    HIPC(hipMemcpyAsync(c->d_kstart, d_kstart, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

extern "C" int opus_llama_prefix(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, float *d_last_logits,
                                 float *d_last_rows, int64_t *epoch, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    if (!d_last_rows || !epoch) return fail(OPUS_EBADARG, "prefix: null last rows / epoch");
    hipStream_t s = (hipStream_t)stream;
    c->h_kstart.clear();
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T));
    const opus_config &g = c->cfg;
    HIPC(hipMemcpyAsync(d_last_rows, c->d_xl, (size_t)B * g.dec_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (d_last_logits)
        HIPC(hipMemcpyAsync(d_last_logits, c->d_logits, (size_t)B * g.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    std::vector<int32_t> kst(B);
    HIPC(hipMemcpyAsync(kst.data(), c->d_kstart, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    c->h_kstart = kst;
    *epoch = c->epoch;
    return OPUS_OK;
}

extern "C" int64_t opus_llama_score_scratch_bytes(const opus_config *cfg, int32_t R, int32_t n) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    if (R < 1 || n < 1 || n > cfg->max_prompt) {
        fail(OPUS_ESHAPE, "score_scratch_bytes: R=%d n=%d (1 <= n <= max_prompt=%d)", R, n, cfg->max_prompt);
        return -1;
    }
    return prefix_scratch_bytes(*cfg, R, n);
}

static int score_continuations_impl(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                    const int32_t *h_lens, const int32_t *h_src, const float *d_last_rows, int32_t P, int64_t epoch,
                                    const int32_t *d_targets, float *d_logprob, void *d_scratch, int64_t scratch_bytes, void *stream) {
    OPC(need_ready(c));
    if (!d_embeds || !h_lens || !h_src || !d_last_rows || !d_targets || !d_logprob || !d_scratch)
        return fail(OPUS_EBADARG, "score_continuations: null pointer");
    const opus_config &g = c->cfg;
    if (R < 1 || n < 1 || n > g.max_prompt)
        return fail(OPUS_ESHAPE, "score_continuations: R=%d rows of n=%d positions (1 <= n <= max_prompt=%d)", R, n, g.max_prompt);
    PrefixSrc ps;
    OPC(resolve_prefix(c, "score_continuations", snap, P, epoch, ps));
    P = ps.P;
    const int Tp = ps.Tp, ctx_cap = g.max_prompt + g.max_new_tokens;
    int64_t N = 0;
    for (int r = 0; r < R; ++r) {
        if (h_src[r] < 0 || h_src[r] >= P) return fail(OPUS_EBADARG, "score_continuations: prefix row %d of row %d outside [0, %d)", h_src[r], r, P);
        if (h_lens[r] < 0 || h_lens[r] > n) return fail(OPUS_ESHAPE, "score_continuations: length %d of row %d outside [0, %d]", h_lens[r], r, n);
        if (Tp - ps.kst[h_src[r]] + n > ctx_cap)
            return fail(OPUS_ESHAPE, "score_continuations: prefix of %d tokens + %d positions exceed the context's %d positions "
                                     "(max_prompt + max_new_tokens)", Tp - ps.kst[h_src[r]], n, ctx_cap);
        N += h_lens[r];
    }
    if (N >= (1ll << 31)) return fail(OPUS_ESHAPE, "score_continuations: %lld scored tokens", (long long)N);
    const int64_t need = prefix_scratch_bytes(g, R, n);
    if (scratch_bytes < need)
        return fail(OPUS_EBADARG, "score_continuations: scratch of %lld bytes, %lld needed (opus_llama_score_scratch_bytes)",
                    (long long)scratch_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int H = g.dec_dim, G = g.dec_heads / g.dec_kv_heads;
    const int64_t Rg_max = prefix_group_rows(g, R, n);
    const int64_t chunk = score_chunk_cap(g, Rg_max * n, true);
    int32_t *tbl = reinterpret_cast<int32_t *>(d_scratch);
    float *rows_f = reinterpret_cast<float *>((char *)d_scratch + align_up((size_t)prefix_table_words(g, Rg_max, n) * sizeof(int32_t)));
    half_t *slab = reinterpret_cast<half_t *>((char *)rows_f + align_up((size_t)chunk * H * sizeof(float)));
    int64_t base = 0;                                               // compact index of the pass's first scored token
    for (int64_t r0 = 0; r0 < R; r0 += Rg_max) {
        const int Rg = (int)std::min<int64_t>(Rg_max, R - r0);
        PrefixTables t;
        build_prefix_tables(g, ps.kst, Tp, h_src + r0, Rg, n, t);
        if (t.nblocks > attn_prefix_max_blocks(Rg, g.max_batch, G, n)) return fail(OPUS_EHIP, "score_continuations: block table overflow");
        // scored rows: token 0 of row r from the prefix's last row (gather index -(p) - 1), token j from position j - 1 of the pass
        int64_t Ng = 0;
        for (int r = 0; r < Rg; ++r) {
            const int L = h_lens[r0 + r];
            if (L > 0) t.w.push_back(-h_src[r0 + r] - 1);
            for (int j = 1; j < L; ++j) t.w.push_back(r * n + j - 1);
            Ng += L;
        }
        if ((int64_t)t.w.size() > prefix_table_words(g, Rg_max, n)) return fail(OPUS_EHIP, "score_continuations: table overflow");
        HIPC(hipMemcpyAsync(tbl, t.w.data(), t.w.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        ContRows cr;
        cr.nkst = tbl + t.nkst;
        cr.nblocks = t.nblocks;
        cr.attn = prefix_params(c, tbl, t, Tp, n, c->d_qkv, nullptr, nullptr, c->d_ctx);
        ps.apply(g, cr);
        const half_t *emb = reinterpret_cast<const half_t *>(d_embeds) + r0 * n * (int64_t)H;
        OPC(prefill(c, s, emb, nullptr, Rg, n, true, &cr));
        c->phase = PH_SCORE;
        for (int64_t k0 = 0; k0 < Ng; k0 += chunk) {
            const int m = (int)std::min<int64_t>(chunk, Ng - k0);
            KL(KC_OTHER, 8.0 * m * H + 4.0 * m,
               launch_gather_rows2(c->d_x, (int64_t)Rg * n, d_last_rows, P, tbl + t.gidx + k0, m, H, rows_f, s));
            OPC(score_rows(c, s, rows_f, m, slab, d_targets + base + k0, d_logprob + base + k0, nullptr));
        }
        base += Ng;
        HIPC(hipStreamSynchronize(s));                              // (the table upload's host buffer is reused by the next pass)
    }
    return OPUS_OK;
}

extern "C" int opus_llama_score_continuations(opus_ctx *c, const void *d_embeds, int32_t R, int32_t n, const int32_t *h_lens,
                                              const int32_t *h_src, const float *d_last_rows, int32_t P, int64_t epoch,
                                              const int32_t *d_targets, float *d_logprob, void *d_scratch, int64_t scratch_bytes,
                                              void *stream) {
    return score_continuations_impl(c, nullptr, d_embeds, R, n, h_lens, h_src, d_last_rows, P, epoch, d_targets, d_logprob, d_scratch,
                                    scratch_bytes, stream);
}

extern "C" int opus_llama_score_continuations_detached(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t R,
                                                       int32_t n, const int32_t *h_lens, const int32_t *h_src, const float *d_last_rows,
                                                       const int32_t *d_targets, float *d_logprob, void *d_scratch,
                                                       int64_t scratch_bytes, void *stream) {
    if (!snap) return fail(OPUS_EBADARG, "score_continuations_detached: null snapshot");
    return score_continuations_impl(c, snap, d_embeds, R, n, h_lens, h_src, d_last_rows, 0, 0, d_targets, d_logprob, d_scratch,
                                    scratch_bytes, stream);
}

// The shared body of opus_debug_attn_prefix / opus_debug_attn_tree (h_par: the tree form, n = 1), after their argument checks:
// seeds layer 0 of the cache, builds and uploads the tables, one timed launch.  Leaves the context without a prefill.
static int debug_attn_prefix_run(opus_ctx *c, const char *who, const void *d_qkv, const void *d_k_hist, const void *d_v_hist,
                                 const int32_t *d_kstart, int P, int Tp, int R, int n, const int32_t *h_src, const int32_t *h_par,
                                 void *d_out, void *stream) {
    const opus_config &g = c->cfg;
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nkv = g.dec_kv_heads, hd = g.dec_head_dim, G = g.dec_heads / nkv;
    std::vector<int32_t> kst(P);
    HIPC(hipMemcpyAsync(kst.data(), d_kstart, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int p = 0; p < P; ++p)
        if (kst[p] < 0 || kst[p] >= Tp) return fail(OPUS_EBADARG, "%s: kstart[%d]=%d outside [0, %d)", who, p, kst[p], Tp);
    c->prefilled = false;                                     // (the cache no longer belongs to a prefill)
    new_epoch(c);
    OPC(seed_cache(c, s, d_k_hist, d_v_hist, d_kstart, P, Tp));
    PrefixTables t;
    build_prefix_tables(g, kst, Tp, h_src, R, n, t);
    const int o_par = (int)t.w.size();
    if (h_par) t.w.insert(t.w.end(), h_par, h_par + R);
    int32_t *d_tbl = nullptr;
    HIPC(hipMalloc((void **)&d_tbl, t.w.size() * sizeof(int32_t)));
    hipError_t e = hipMemcpyAsync(d_tbl, t.w.data(), t.w.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
    AttnPrefixParams a = prefix_params(c, d_tbl, t, Tp, n, (const half_t *)d_qkv, c->kc, c->vc, (half_t *)d_out);
    if (h_par) a.par = d_tbl + o_par;
    c->phase = PH_SCORE;
    if (e == hipSuccess) {
        Timed tm(c, s, KC_ATTN_PREFILL, 2.0 * R * n * (double)(G + 2) * nkv * hd * 2 + 4.0 * t.nblocks * nkv * hd * Tp,
                 4.0 * R * n * (double)G * nkv * hd * (Tp + n));
        e = launch_attn_prefix(a, t.nblocks, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_tbl);
    if (e != hipSuccess) return fail(OPUS_EHIP, "%s failed: %s", who, hipGetErrorString(e));
    return OPUS_OK;
}

// attn_prefix_kernel alone, as opus_llama_score_continuations launches it, on layer 0 of this context's KV cache: the prefix
// d_k_hist / d_v_hist [P, kv heads, Tp, hd] (keys rotated, as the cache holds them) is copied into slots 0 .. Tp - 1 and d_kstart
// [P] into the context's kstart; d_qkv [R n, (heads + 2 kv) hd]: the continuation rows' projections, q and k already rotated;
// h_src [R] (host): prefix row of every continuation row.  d_out [R n, heads hd].  Leaves the context without a prefill.
extern "C" int opus_debug_attn_prefix(opus_ctx *c, const void *d_qkv, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                                      int32_t P, int32_t Tp, int32_t R, int32_t n, const int32_t *h_src, void *d_out, void *stream) {
    if (!c || !d_qkv || !d_k_hist || !d_v_hist || !d_kstart || !h_src || !d_out) return fail(OPUS_EBADARG, "debug_attn_prefix: null pointer");
    const opus_config &g = c->cfg;
    if (P < 1 || P > g.max_batch || Tp < 1 || Tp > g.max_prompt || R < 1 || n < 1)
        return fail(OPUS_ESHAPE, "debug_attn_prefix: P=%d Tp=%d R=%d n=%d exceed the context (%d, %d)", P, Tp, R, n, g.max_batch, g.max_prompt);
    for (int r = 0; r < R; ++r)
        if (h_src[r] < 0 || h_src[r] >= P) return fail(OPUS_EBADARG, "debug_attn_prefix: prefix row %d of row %d outside [0, %d)", h_src[r], r, P);
    return debug_attn_prefix_run(c, "debug_attn_prefix", d_qkv, d_k_hist, d_v_hist, d_kstart, P, Tp, R, n, h_src, nullptr, d_out, stream);
}

// ------------------------------------------------------------------------------------------------ trie scoring
// opus_llama_score_tree = one pass of a token trie's nodes behind the cached prefix: every row is one new position (a node) that
// attends to its prefix row's cache slots and to its own ancestors in the pass (attn_prefix_kernel's tree form).  The planning (which nodes,
// which order, which pass) is the caller's (opus-pllm_amd/constraint.py, plan_trie_score); this entry checks every table it is
// given before anything reaches a kernel.
enum { TREE_MAX_DEPTH = 64 };

extern "C" int64_t opus_llama_dec_rows_cap(const opus_config *cfg) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    return dec_rows_cap(*cfg);
}
extern "C" int32_t opus_llama_tree_max_depth(void) { return TREE_MAX_DEPTH; }

// scored rows per lm_head chunk: the slab's cap, and never more rows than the activation buffers hold (the scored list of a full
// pass is up to max_batch entries longer than the pass: the prefix rows' last positions)
static int64_t tree_chunk(const opus_config &g, int64_t n_score) {
    return score_chunk_cap(g, std::min<int64_t>(std::max<int64_t>(n_score, 1), dec_rows_cap(g)), true);
}
static int64_t tree_table_words(const opus_config &g, int64_t rows, int64_t n_score, int64_t n_edges, int64_t n_stops, int64_t n_ids,
                                int64_t n_sets) {
    const int G = g.dec_heads / g.dec_kv_heads;
    return (int64_t)g.max_batch + 1 + 3 * rows + 2 * (int64_t)attn_prefix_max_blocks((int)rows, g.max_batch, G, 1) + n_score +
           3 * n_edges + 3 * n_stops + n_ids + n_sets + 1 + tree_chunk(g, n_score);
}
static int64_t tree_scratch_bytes(const opus_config &g, int64_t rows, int64_t n_score, int64_t n_edges, int64_t n_stops, int64_t n_ids,
                                  int64_t n_sets) {
    const int64_t chunk = tree_chunk(g, n_score);
    return (int64_t)align_up((size_t)tree_table_words(g, rows, n_score, n_edges, n_stops, n_ids, n_sets) * sizeof(int32_t)) +
           score_chunk_bytes(g, chunk, true) + 2 * (int64_t)align_up((size_t)chunk * sizeof(float));
}

extern "C" int64_t opus_llama_score_tree_scratch_bytes(const opus_config *cfg, int32_t rows, int32_t n_score, int32_t n_edges,
                                                       int32_t n_stops, int32_t n_stop_ids, int32_t n_stop_sets) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    if (rows < 0 || rows > dec_rows_cap(*cfg) || n_score < 0 || n_edges < 0 || n_stops < 0 || n_stop_ids < 0 || n_stop_sets < 0) {
        fail(OPUS_ESHAPE, "score_tree_scratch_bytes: rows=%d (0 .. %lld) scored=%d edges=%d stops=%d ids=%d sets=%d", rows,
             (long long)dec_rows_cap(*cfg), n_score, n_edges, n_stops, n_stop_ids, n_stop_sets);
        return -1;
    }
    return tree_scratch_bytes(*cfg, rows, n_score, n_edges, n_stops, n_stop_ids, n_stop_sets);
}

// the rows' tables of one pass: every parent earlier in the pass, in the same prefix row, one level up
static int check_tree_rows(const char *who, int rows, int P, const int32_t *h_src, const int32_t *h_par, const int32_t *h_depth) {
    for (int r = 0; r < rows; ++r) {
        if (h_src[r] < 0 || h_src[r] >= P) return fail(OPUS_EBADARG, "%s: prefix row %d of row %d outside [0, %d)", who, h_src[r], r, P);
        if (h_depth[r] < 1 || h_depth[r] > TREE_MAX_DEPTH)
            return fail(OPUS_ESHAPE, "%s: depth %d of row %d outside [1, %d]", who, h_depth[r], r, (int)TREE_MAX_DEPTH);
        const int pa = h_par[r];
        if (h_depth[r] == 1 ? pa != -1 : (pa < 0 || pa >= r || h_src[pa] != h_src[r] || h_depth[pa] != h_depth[r] - 1))
            return fail(OPUS_EBADARG, "%s: parent %d of row %d (depth %d) is not an earlier row of its prefix row one level up", who, pa,
                        r, h_depth[r]);
    }
    return OPUS_OK;
}

static int score_tree_impl(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t rows, const int32_t *h_src,
                           const int32_t *h_par, const int32_t *h_depth, int32_t n_score, const int32_t *h_score_src, int32_t n_edges,
                           const int32_t *h_edge_row, const int32_t *h_edge_tok, const int32_t *h_edge_slot, int32_t n_stops,
                           const int32_t *h_stop_row, const int32_t *h_stop_set, const int32_t *h_stop_slot, int32_t n_stop_ids,
                           const int32_t *h_stop_ids, int32_t n_stop_sets, const int32_t *h_stop_off, const float *d_last_rows,
                           int32_t P, int64_t epoch, float *d_node_lp, float *d_stop_lp, int64_t n_slots, void *d_scratch,
                           int64_t scratch_bytes, void *stream) {
    OPC(need_ready(c));
    const opus_config &g = c->cfg;
    if (rows < 0 || rows > dec_rows_cap(g) || n_score < 0 || n_edges < 0 || n_stops < 0 || n_stop_ids < 0 || n_stop_sets < 0 || n_slots < 1)
        return fail(OPUS_ESHAPE, "score_tree: rows=%d (0 .. %lld) scored=%d edges=%d stops=%d ids=%d sets=%d slots=%lld", rows,
                    (long long)dec_rows_cap(g), n_score, n_edges, n_stops, n_stop_ids, n_stop_sets, (long long)n_slots);
    if (!d_last_rows || !d_node_lp || !d_scratch || (rows && (!d_embeds || !h_src || !h_par || !h_depth)) || (n_score && !h_score_src) ||
        (n_edges && (!h_edge_row || !h_edge_tok || !h_edge_slot)) ||
        (n_stops && (!h_stop_row || !h_stop_set || !h_stop_slot || !h_stop_ids || !h_stop_off || !d_stop_lp)))
        return fail(OPUS_EBADARG, "score_tree: null pointer");
    PrefixSrc ps;
    OPC(resolve_prefix(c, "score_tree", snap, P, epoch, ps));
    P = ps.P;
    const int Tp = ps.Tp, ctx_cap = g.max_prompt + g.max_new_tokens, V = g.dec_vocab, H = g.dec_dim;
    OPC(check_tree_rows("score_tree", rows, P, h_src, h_par, h_depth));
    for (int r = 0; r < rows; ++r)
        if (Tp - ps.kst[h_src[r]] + h_depth[r] > ctx_cap)
            return fail(OPUS_ESHAPE, "score_tree: prefix of %d tokens + depth %d exceed the context's %d positions (max_prompt + "
                                     "max_new_tokens)", Tp - ps.kst[h_src[r]], h_depth[r], ctx_cap);
    for (int k = 0; k < n_score; ++k)
        if (h_score_src[k] >= rows || h_score_src[k] < -P)
            return fail(OPUS_EBADARG, "score_tree: scored source %d of entry %d outside [-%d, %d)", h_score_src[k], k, P, rows);
    for (int e = 0; e < n_edges; ++e)
        if (h_edge_row[e] < (e ? h_edge_row[e - 1] : 0) || h_edge_row[e] >= n_score || h_edge_tok[e] < 0 || h_edge_tok[e] >= V ||
            h_edge_slot[e] < 0 || h_edge_slot[e] >= n_slots)
            return fail(OPUS_EBADARG, "score_tree: edge %d (scored row %d, id %d, slot %d): rows ascending below %d, ids below %d, "
                                      "slots below %lld", e, h_edge_row[e], h_edge_tok[e], h_edge_slot[e], n_score, V, (long long)n_slots);
    if (n_stops) {
        if (n_stop_sets < 1 || h_stop_off[0] != 0 || h_stop_off[n_stop_sets] != n_stop_ids)
            return fail(OPUS_EBADARG, "score_tree: stop sets: offsets must run from 0 to %d", n_stop_ids);
        for (int k = 0; k < n_stop_sets; ++k)
            if (h_stop_off[k + 1] <= h_stop_off[k]) return fail(OPUS_EBADARG, "score_tree: stop set %d is empty or out of order", k);
        for (int k = 0; k < n_stop_ids; ++k)
            if (h_stop_ids[k] < 0 || h_stop_ids[k] >= V) return fail(OPUS_EBADARG, "score_tree: stop id %d outside [0, %d)", h_stop_ids[k], V);
        for (int k = 0; k < n_stops; ++k)
            if (h_stop_row[k] < (k ? h_stop_row[k - 1] : 0) || h_stop_row[k] >= n_score || h_stop_set[k] < 0 ||
                h_stop_set[k] >= n_stop_sets || h_stop_slot[k] < 0 || h_stop_slot[k] >= n_slots)
                return fail(OPUS_EBADARG, "score_tree: stop entry %d (scored row %d, set %d, slot %d)", k, h_stop_row[k], h_stop_set[k],
                            h_stop_slot[k]);
    }
    const int64_t need = tree_scratch_bytes(g, rows, n_score, n_edges, n_stops, n_stop_ids, n_stop_sets);
    if (scratch_bytes < need)
        return fail(OPUS_EBADARG, "score_tree: scratch of %lld bytes, %lld needed (opus_llama_score_tree_scratch_bytes)",
                    (long long)scratch_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int G = g.dec_heads / g.dec_kv_heads;
    const int64_t chunk = tree_chunk(g, n_score);
    PrefixTables t;
    build_prefix_tables(g, ps.kst, Tp, h_src, rows, 1, t);
    if (t.nblocks > attn_prefix_max_blocks(rows, g.max_batch, G, 1)) return fail(OPUS_EHIP, "score_tree: block table overflow");
    for (int r = 0; r < rows; ++r) t.w[t.nkst + r] -= h_depth[r] - 1;      // position of a node at depth d: Tp - kstart[p] + d - 1
    auto put = [&](const int32_t *src, int64_t n) {
        const int at = (int)t.w.size();
        if (n > 0) t.w.insert(t.w.end(), src, src + n);
        return at;
    };
    const int o_par = put(h_par, rows), o_src = put(h_score_src, n_score);
    const int o_er = put(h_edge_row, n_edges), o_et = put(h_edge_tok, n_edges), o_es = put(h_edge_slot, n_edges);
    const int o_sr = put(h_stop_row, n_stops), o_ss = put(h_stop_set, n_stops), o_sl = put(h_stop_slot, n_stops);
    const int o_ids = put(h_stop_ids, n_stops ? n_stop_ids : 0), o_off = put(h_stop_off, n_stops ? n_stop_sets + 1 : 0);
    const int o_neg = (int)t.w.size();
    t.w.insert(t.w.end(), (size_t)chunk, -1);                                // xent's targets: none counted, the lse is what is used
    const int64_t words = tree_table_words(g, rows, n_score, n_edges, n_stops, n_stop_ids, n_stop_sets);
    if ((int64_t)t.w.size() > words) return fail(OPUS_EHIP, "score_tree: table overflow");
    int32_t *tbl = reinterpret_cast<int32_t *>(d_scratch);
    float *rows_f = reinterpret_cast<float *>((char *)d_scratch + align_up((size_t)words * sizeof(int32_t)));
    half_t *slab = reinterpret_cast<half_t *>((char *)rows_f + align_up((size_t)chunk * H * sizeof(float)));
    float *lse = reinterpret_cast<float *>((char *)slab + align_up((size_t)chunk * V * sizeof(half_t)));
    float *lp_none = reinterpret_cast<float *>((char *)lse + align_up((size_t)chunk * sizeof(float)));
    HIPC(hipMemcpyAsync(tbl, t.w.data(), t.w.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (rows > 0) {
        ContRows cr;
        cr.nkst = tbl + t.nkst;
        cr.nblocks = t.nblocks;
        cr.attn = prefix_params(c, tbl, t, Tp, 1, c->d_qkv, nullptr, nullptr, c->d_ctx);
        cr.attn.par = tbl + o_par;
        ps.apply(g, cr);
        OPC(prefill(c, s, reinterpret_cast<const half_t *>(d_embeds), nullptr, rows, 1, true, &cr));
    }
    c->phase = PH_SCORE;
    int e0 = 0, k0s = 0;
    for (int64_t k0 = 0; k0 < n_score; k0 += chunk) {
        const int m = (int)std::min<int64_t>(chunk, n_score - k0);
        int e1 = e0, k1s = k0s;
        while (e1 < n_edges && h_edge_row[e1] < k0 + m) ++e1;
        while (k1s < n_stops && h_stop_row[k1s] < k0 + m) ++k1s;
        KL(KC_OTHER, 8.0 * m * H + 4.0 * m, launch_gather_rows2(c->d_x, rows, d_last_rows, P, tbl + o_src + k0, m, H, rows_f, s));
        OPC(score_rows(c, s, rows_f, m, slab, tbl + o_neg, lp_none, lse));
        KL(KC_XENT, 14.0 * (e1 - e0) + 16.0 * (k1s - k0s),
           launch_tree_edges(slab, V, lse, (int)k0, tbl + o_er + e0, tbl + o_et + e0, tbl + o_es + e0, e1 - e0, d_node_lp,
                             tbl + o_sr + k0s, tbl + o_ss + k0s, tbl + o_sl + k0s, k1s - k0s, tbl + o_ids, tbl + o_off, d_stop_lp, s));
        e0 = e1;
        k0s = k1s;
    }
    HIPC(hipStreamSynchronize(s));                                          // (the host tables are the caller's: they may go away)
    return OPUS_OK;
}

extern "C" int opus_llama_score_tree(opus_ctx *c, const void *d_embeds, int32_t rows, const int32_t *h_src, const int32_t *h_par,
                                     const int32_t *h_depth, int32_t n_score, const int32_t *h_score_src, int32_t n_edges,
                                     const int32_t *h_edge_row, const int32_t *h_edge_tok, const int32_t *h_edge_slot, int32_t n_stops,
                                     const int32_t *h_stop_row, const int32_t *h_stop_set, const int32_t *h_stop_slot,
                                     int32_t n_stop_ids, const int32_t *h_stop_ids, int32_t n_stop_sets, const int32_t *h_stop_off,
                                     const float *d_last_rows, int32_t P, int64_t epoch, float *d_node_lp, float *d_stop_lp,
                                     int64_t n_slots, void *d_scratch, int64_t scratch_bytes, void *stream) {
    return score_tree_impl(c, nullptr, d_embeds, rows, h_src, h_par, h_depth, n_score, h_score_src, n_edges, h_edge_row, h_edge_tok,
                           h_edge_slot, n_stops, h_stop_row, h_stop_set, h_stop_slot, n_stop_ids, h_stop_ids, n_stop_sets, h_stop_off,
                           d_last_rows, P, epoch, d_node_lp, d_stop_lp, n_slots, d_scratch, scratch_bytes, stream);
}

extern "C" int opus_llama_score_tree_detached(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t rows,
                                              const int32_t *h_src, const int32_t *h_par, const int32_t *h_depth, int32_t n_score,
                                              const int32_t *h_score_src, int32_t n_edges, const int32_t *h_edge_row,
                                              const int32_t *h_edge_tok, const int32_t *h_edge_slot, int32_t n_stops,
                                              const int32_t *h_stop_row, const int32_t *h_stop_set, const int32_t *h_stop_slot,
                                              int32_t n_stop_ids, const int32_t *h_stop_ids, int32_t n_stop_sets,
                                              const int32_t *h_stop_off, const float *d_last_rows, float *d_node_lp, float *d_stop_lp,
                                              int64_t n_slots, void *d_scratch, int64_t scratch_bytes, void *stream) {
    if (!snap) return fail(OPUS_EBADARG, "score_tree_detached: null snapshot");
    return score_tree_impl(c, snap, d_embeds, rows, h_src, h_par, h_depth, n_score, h_score_src, n_edges, h_edge_row, h_edge_tok,
                           h_edge_slot, n_stops, h_stop_row, h_stop_set, h_stop_slot, n_stop_ids, h_stop_ids, n_stop_sets, h_stop_off,
                           d_last_rows, 0, 0, d_node_lp, d_stop_lp, n_slots, d_scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ detached prefixes
// opus_llama_prefix_export copies a prefill's K / V out of the cache (a snapshot the caller owns); opus_llama_prefill_behind puts
// snapshot rows back under R suffix rows and leaves the context as after a prefill of the concatenated prompts.

static int64_t prefix_snap_halfs(const opus_config &g, int64_t rows, int64_t T) {
    return (int64_t)g.dec_layers * rows * g.dec_kv_heads * T * g.dec_head_dim;
}

extern "C" int64_t opus_llama_prefix_bytes(const opus_config *cfg, int32_t P, int32_t Tp) {
    if (check_cfg(cfg) != OPUS_OK) return -1;
    if (P < 1 || Tp < 1 || P > cfg->max_batch || Tp > cfg->max_prompt + cfg->max_new_tokens) {
        fail(OPUS_ESHAPE, "prefix_bytes: P=%d Tp=%d (1 .. max_batch=%d rows, 1 .. %d slots)", P, Tp, cfg->max_batch,
             cfg->max_prompt + cfg->max_new_tokens);
        return -1;
    }
    return 2 * prefix_snap_halfs(*cfg, P, Tp) * (int64_t)sizeof(half_t);
}

extern "C" int opus_llama_prefix_export(opus_ctx *c, int64_t epoch, int32_t R, int32_t T, void *d_k, void *d_v, int32_t *d_kstart,
                                        void *stream) {
    OPC(need_ready(c));
    if (!d_k || !d_v) return fail(OPUS_EBADARG, "prefix_export: null pointer");
    const opus_config &g = c->cfg;
    if (!c->prefilled || epoch != c->epoch)
        return fail(OPUS_ESTATE, "prefix_export: the epoch is not this context's current one (a later call prefilled or permuted the "
                                 "cache, or it belongs to another context)");
    if (R < 1 || R > g.max_batch || T < 1 || T > g.max_prompt + g.max_new_tokens)
        return fail(OPUS_ESHAPE, "prefix_export: R=%d rows of T=%d slots (1 .. max_batch=%d, 1 .. %d)", R, T, g.max_batch,
                    g.max_prompt + g.max_new_tokens);
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    KL(KC_OTHER, 4.0 * (double)prefix_snap_halfs(g, R, T) * sizeof(half_t),
       launch_kv_export(c->kc, c->vc, c->cache_sl, c->cache_sb, c->cache_sh, g.dec_layers, R, g.dec_kv_heads, T, g.dec_head_dim,
                        (half_t *)d_k, (half_t *)d_v, s));
    if (d_kstart) HIPC(hipMemcpyAsync(d_kstart, c->d_kstart, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

// words of the behind pass's device tables: PrefixTables (+ workgroup table) | lens [R] | gather index [R]
static int64_t behind_table_words(const opus_config &g) {
    const int G = g.dec_heads / g.dec_kv_heads;
    const int64_t nb = dec_rows_cap(g) * G / 128 + g.max_batch + 1;        // (attn_prefix_max_blocks for the largest pass)
    return (int64_t)g.max_batch + 1 + 4 * (int64_t)g.max_batch + 2 * nb;
}

// The prefill of opus_llama_prefill_behind / opus_generate_scored_behind, after need_ready: checks, tables, kv_place, the suffix
// pass (prefill()'s layer loop with continuation rows that also append to the cache), the rows' last positions, lm_head, state.
struct BehindArgs {
    const opus_prefix_snap *snap;
    const int32_t *h_lens, *h_src;
};
static int prefill_behind(opus_ctx *c, hipStream_t s, const BehindArgs &b, const half_t *embeds, int R, int n,
                          std::vector<int32_t> *nks_out = nullptr) {
    const opus_config &g = c->cfg;
    if (!b.snap || !b.h_lens || !b.h_src || !embeds) return fail(OPUS_EBADARG, "prefill_behind: null pointer");
    PrefixSrc ps;
    OPC(resolve_prefix(c, "prefill_behind", b.snap, 0, 0, ps));
    const int P = ps.P, Tp = ps.Tp, H = g.dec_dim, G = g.dec_heads / g.dec_kv_heads;
    if (R < 1 || R > g.max_batch)
        return fail(OPUS_ESHAPE, "prefill_behind: R=%d decoder rows, the context holds max_batch=%d", R, g.max_batch);
    if (n < 1 || Tp + n > g.max_prompt)
        return fail(OPUS_ESHAPE, "prefill_behind: prefix of %d slots + suffix of %d positions = %d, the context holds max_prompt=%d", Tp, n,
                    Tp + n, g.max_prompt);
    if ((int64_t)R * n > dec_rows_cap(g))
        return fail(OPUS_ESHAPE, "prefill_behind: R x n = %d x %d suffix positions, the prefill buffers hold %lld", R, n,
                    (long long)dec_rows_cap(g));
    for (int r = 0; r < R; ++r) {
        if (b.h_src[r] < 0 || b.h_src[r] >= P) return fail(OPUS_EBADARG, "prefill_behind: prefix row %d of row %d outside [0, %d)", b.h_src[r], r, P);
        if (b.h_lens[r] < 1 || b.h_lens[r] > n) return fail(OPUS_ESHAPE, "prefill_behind: suffix length %d of row %d outside [1, %d]", b.h_lens[r], r, n);
    }
    if (!c->behind_tbl) HIPC(hipMalloc((void **)&c->behind_tbl, (size_t)behind_table_words(g) * sizeof(int32_t)));
    PrefixTables t;
    build_prefix_tables(g, ps.kst, Tp, b.h_src, R, n, t);
    if (t.nblocks > attn_prefix_max_blocks(R, g.max_batch, G, n)) return fail(OPUS_EHIP, "prefill_behind: block table overflow");
    const int o_lens = (int)t.w.size();
    t.w.insert(t.w.end(), b.h_lens, b.h_lens + R);
    const int o_last = (int)t.w.size();
    std::vector<int32_t> nks(R);
    for (int r = 0; r < R; ++r) {
        t.w.push_back(r * n + b.h_lens[r] - 1);                               // the row's last real position in the pass
        nks[r] = ps.kst[b.h_src[r]] + n - b.h_lens[r];                        // kstart' = kstart[p] + d_r
    }
    if ((int64_t)t.w.size() > behind_table_words(g)) return fail(OPUS_EHIP, "prefill_behind: table overflow");
    int32_t *tbl = c->behind_tbl;
    new_epoch(c);
    c->prefilled = false;                                                     // (until the pass is enqueued whole)
    c->cur_B = 0;
    c->h_kstart.clear();
    c->phase = PH_PREFILL;
    HIPC(launch_upload_i32(t.w.data(), (int)t.w.size(), tbl, s));
    HIPC(launch_upload_i32(nks.data(), R, c->d_kstart, s));
    KvPlaceParams kp;
    kp.snap_k = reinterpret_cast<const half_t *>(b.snap->d_k); kp.snap_v = reinterpret_cast<const half_t *>(b.snap->d_v);
    kp.kstart = b.snap->d_kstart; kp.P = P; kp.Tp = Tp; kp.kc = c->kc; kp.vc = c->vc;
    kp.cache_sl = c->cache_sl; kp.cache_sb = c->cache_sb; kp.cache_sh = c->cache_sh;
    kp.list = tbl + t.list; kp.off = tbl + t.off; kp.new_kstart = c->d_kstart;
    kp.layers = g.dec_layers; kp.nkv = g.dec_kv_heads; kp.hd = g.dec_head_dim;
    double placed = 0.0, read = 0.0;                                          // slots written / read, for the launch's byte count
    for (int r = 0; r < R; ++r) placed += Tp - ps.kst[b.h_src[r]];
    for (int p = 0; p < P; ++p) read += t.w[t.off + p + 1] > t.w[t.off + p] ? Tp - ps.kst[p] : 0;
    // timed under phase "other": opus_timing_get("other", "other") behind this call is the placement launch alone (its own
    // dispatch timestamps), apart from the prefill phase's class totals
    c->phase = PH_OTHER;
    KL(KC_OTHER, (placed + read) * 2.0 * g.dec_layers * g.dec_kv_heads * g.dec_head_dim * sizeof(half_t), launch_kv_place(kp, s));
    c->phase = PH_PREFILL;
    ContRows cr;
    cr.nkst = tbl + t.nkst;
    cr.nblocks = t.nblocks;
    cr.attn = prefix_params(c, tbl, t, Tp, n, c->d_qkv, nullptr, nullptr, c->d_ctx);
    ps.apply(g, cr);
    cr.app_lens = tbl + o_lens;
    OPC(prefill(c, s, embeds, nullptr, R, n, true, &cr));
    c->phase = PH_PREFILL;
    // every position ran through the last layer (the continuation-row form keeps all rows): the rows' last real positions -> d_xl
    KL(KC_OTHER, 8.0 * R * H + 4.0 * R, launch_gather_rows(c->d_x, tbl + o_last, R, (int64_t)R * n, H, c->d_xl, s));
    if (g.dec_arch == 1) {
        OPC(lm_head_opt(c, s, R));
    } else {
        ResidShadow none;
        OPC(lm_head(c, s, none, R));
    }
    OPC(reset_step(c, s, Tp + n));
    c->cur_B = R;
    c->cur_T = Tp + n;
    c->prefilled = true;
    ++c->prefills_behind;
    if (nks_out) nks_out->swap(nks);                                          // (opus_llama_prefix_behind: the rows' kstart on the host)
    return OPUS_OK;
}

extern "C" int opus_llama_prefill_behind(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                         const int32_t *h_lens, const int32_t *h_src, float *d_last_logits, int64_t *epoch,
                                         void *stream) {
    OPC(need_ready(c));
    hipStream_t s = (hipStream_t)stream;
    OPC(prefill_behind(c, s, BehindArgs{snap, h_lens, h_src}, (const half_t *)d_embeds, R, n));
    if (d_last_logits)
        HIPC(hipMemcpyAsync(d_last_logits, c->d_logits, (size_t)R * c->cfg.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (epoch) *epoch = c->epoch;
    return OPUS_OK;
}

// opus_llama_prefill_behind that also hands out the rows' final residual (taken where opus_llama_prefix takes it) and keeps the
// rows' kstart on the host: the context then holds a live prefix of R rows x Tp + n slots, as after opus_llama_prefix on the
// concatenated prompts.
extern "C" int opus_llama_prefix_behind(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                        const int32_t *h_lens, const int32_t *h_src, float *d_last_logits, float *d_last_rows,
                                        int64_t *epoch, void *stream) {
    OPC(need_ready(c));
    if (!d_last_rows || !epoch) return fail(OPUS_EBADARG, "prefix_behind: null last rows / epoch");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> nks;
    OPC(prefill_behind(c, s, BehindArgs{snap, h_lens, h_src}, (const half_t *)d_embeds, R, n, &nks));
    const opus_config &g = c->cfg;
    HIPC(hipMemcpyAsync(d_last_rows, c->d_xl, (size_t)R * g.dec_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (d_last_logits)
        HIPC(hipMemcpyAsync(d_last_logits, c->d_logits, (size_t)R * g.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPC(hipStreamSynchronize(s));
    c->h_kstart = nks;
    *epoch = c->epoch;
    return OPUS_OK;
}

// Ragged copy-out of the cache a decode loop left: row r's window kstart[r] .. T0 + h_keep[r] - 1, right-aligned in a snapshot of
// Tp_out slots (kv_export_rows_kernel).  Reads the step word and kstart back (one synchronisation); changes nothing in the context.
extern "C" int opus_llama_prefix_export_rows(opus_ctx *c, int32_t R, const int32_t *h_keep, int32_t Tp_out, void *d_k, void *d_v,
                                             int32_t *d_kstart_out, void *stream) {
    OPC(need_ready(c));
    if (!h_keep || !d_k || !d_v || !d_kstart_out) return fail(OPUS_EBADARG, "prefix_export_rows: null pointer");
    const opus_config &g = c->cfg;
    if (!c->prefilled) return fail(OPUS_ESTATE, "prefix_export_rows: the context holds no prefill");
    if (c->st.on) return fail(OPUS_ESTATE, "prefix_export_rows: a continuous session is open on this context");
    if (R != c->cur_B) return fail(OPUS_ESHAPE, "prefix_export_rows: R=%d, the last step ran %d rows", R, c->cur_B);
    hipStream_t s = (hipStream_t)stream;
    int32_t steps = 0;
    std::vector<int32_t> kst(R), nks(R);
    HIPC(hipMemcpyAsync(&steps, c->d_step, sizeof(steps), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(kst.data(), c->d_kstart, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int T0 = c->cur_T;
    if (steps < 0 || steps > g.max_new_tokens || T0 < 1 || T0 > g.max_prompt)
        return fail(OPUS_ESTATE, "prefix_export_rows: step word %d / %d prompt slots outside the cache", steps, T0);
    int maxL = 0;
    for (int r = 0; r < R; ++r) {
        if (h_keep[r] < 0 || h_keep[r] > steps)
            return fail(OPUS_ESHAPE, "prefix_export_rows: h_keep[%d]=%d outside [0, %d decode steps]", r, h_keep[r], steps);
        if (kst[r] < 0 || kst[r] >= T0) return fail(OPUS_ESTATE, "prefix_export_rows: kstart[%d]=%d outside [0, %d)", r, kst[r], T0);
        maxL = std::max(maxL, T0 - kst[r] + h_keep[r]);
    }
    if (Tp_out < maxL || Tp_out > g.max_prompt + g.max_new_tokens)
        return fail(OPUS_ESHAPE, "prefix_export_rows: Tp_out=%d (the longest window holds %d slots; at most %d)", Tp_out, maxL,
                    g.max_prompt + g.max_new_tokens);
    double slots = 0.0;
    for (int r = 0; r < R; ++r) {
        nks[r] = Tp_out - (T0 - kst[r] + h_keep[r]);
        slots += Tp_out - nks[r];
    }
    HIPC(launch_upload_i32(nks.data(), R, d_kstart_out, s));
    KvExportRowsParams p;
    p.kc = c->kc; p.vc = c->vc; p.cache_sl = c->cache_sl; p.cache_sb = c->cache_sb; p.cache_sh = c->cache_sh;
    p.kstart = c->d_kstart; p.nks = d_kstart_out; p.R = R; p.Tp = Tp_out;
    p.snap_k = (half_t *)d_k; p.snap_v = (half_t *)d_v; p.layers = g.dec_layers; p.nkv = g.dec_kv_heads; p.hd = g.dec_head_dim;
    const int phase = c->phase;
    c->phase = PH_OTHER;
    // bytes: the windows read, the whole snapshot written
    const double per_slot = 2.0 * g.dec_layers * g.dec_kv_heads * g.dec_head_dim * sizeof(half_t);
    KL(KC_OTHER, (slots + (double)R * Tp_out) * per_slot, launch_kv_export_rows(p, s));
    c->phase = phase;
    return OPUS_OK;
}

extern "C" int opus_trie_path_sums(opus_ctx *c, const float *d_node_lp, const int32_t *d_trie, const int32_t *d_par,
                                   const int32_t *d_depth, const int32_t *d_member_node, int32_t P, int32_t M, int32_t ld_nodes,
                                   float *d_member_lp, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!d_node_lp || !d_trie || !d_par || !d_depth || !d_member_node || !d_member_lp) return fail(OPUS_EBADARG, "trie_path_sums: null pointer");
    if (P < 1 || M < 1 || ld_nodes < 2) return fail(OPUS_ESHAPE, "trie_path_sums: P=%d M=%d nodes=%d", P, M, ld_nodes);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_SCORE;
    KL(KC_OTHER, 12.0 * P * M, launch_tree_path_sums(d_node_lp, d_trie, d_par, d_depth, d_member_node, P, M, ld_nodes, d_member_lp, s));
    return OPUS_OK;
}

// attn_prefix_kernel's tree form alone, as opus_llama_score_tree launches it, on layer 0 of this context's KV cache: the arguments
// of opus_debug_attn_prefix with one position per row (d_qkv [R, (heads + 2 kv) hd]) and h_par / h_depth [R] (host): the parent row
// of every row (-1 at depth 1; an earlier row of the same prefix row one level up).  d_out [R, heads hd].
extern "C" int opus_debug_attn_tree(opus_ctx *c, const void *d_qkv, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                                    int32_t P, int32_t Tp, int32_t R, const int32_t *h_src, const int32_t *h_par, const int32_t *h_depth,
                                    void *d_out, void *stream) {
    if (!c || !d_qkv || !d_k_hist || !d_v_hist || !d_kstart || !h_src || !h_par || !h_depth || !d_out)
        return fail(OPUS_EBADARG, "debug_attn_tree: null pointer");
    const opus_config &g = c->cfg;
    if (P < 1 || P > g.max_batch || Tp < 1 || Tp > g.max_prompt || R < 1)
        return fail(OPUS_ESHAPE, "debug_attn_tree: P=%d Tp=%d R=%d exceed the context (%d, %d)", P, Tp, R, g.max_batch, g.max_prompt);
    OPC(check_tree_rows("debug_attn_tree", R, P, h_src, h_par, h_depth));
    return debug_attn_prefix_run(c, "debug_attn_tree", d_qkv, d_k_hist, d_v_hist, d_kstart, P, Tp, R, 1, h_src, h_par, d_out, stream);
}

// opus_generate_scored's outputs (StepPlan::outs)
enum { GEN_LOGPROBS = 1, GEN_SCORES = 2, GEN_LOGITS = 4, GEN_TOPLP = 8 };

static int ensure_gen_mem(opus_ctx *c) {
    if (c->gen_mem) return OPUS_OK;
    const size_t B = c->cfg.max_batch;
    const size_t o_ps = align_up(sizeof(GenOutDesc)), o_thr = o_ps + align_up(APART * B * sizeof(float));
    HIPC(hipMalloc((void **)&c->gen_mem, o_thr + align_up(B * sizeof(float))));
    c->d_gen = reinterpret_cast<GenOutDesc *>(c->gen_mem);
    c->d_gpsum = reinterpret_cast<float *>(c->gen_mem + o_ps);
    c->d_gthr = reinterpret_cast<float *>(c->gen_mem + o_thr);
    return OPUS_OK;
}

static int ensure_topk_mem(opus_ctx *c) {
    if (c->topk_mem) return OPUS_OK;
    const size_t R = c->topk_rows(), o_lse = align_up(R * APART * TOPK_MAX * sizeof(uint64_t));
    HIPC(hipMalloc((void **)&c->topk_mem, o_lse + align_up(R * sizeof(float))));
    c->d_tcand = reinterpret_cast<uint64_t *>(c->topk_mem);
    c->d_tlse = reinterpret_cast<float *>(c->topk_mem + o_lse);
    return OPUS_OK;
}

// sampling warpers on: the descriptor and the rows' band bounds exist, and the descriptor holds the host setting (stream order)
static int upload_warpers(opus_ctx *c, hipStream_t s) {
    if (!c->warp_mem) {
        const size_t B = c->cfg.max_batch, o_lo = align_up(sizeof(SamplingWarpers)), rows = align_up(B * sizeof(float));
        HIPC(hipMalloc((void **)&c->warp_mem, o_lo + 2 * rows));
        c->d_warp = reinterpret_cast<SamplingWarpers *>(c->warp_mem);
        c->d_wlo = reinterpret_cast<float *>(c->warp_mem + o_lo);
        c->d_whi = reinterpret_cast<float *>(c->warp_mem + o_lo + rows);
    }
    HIPC(launch_upload_i32(reinterpret_cast<const int32_t *>(&c->h_warp), (int)(sizeof(SamplingWarpers) / sizeof(int32_t)),
                           reinterpret_cast<int32_t *>(c->d_warp), s));
    return OPUS_OK;
}

static int ensure_lproc_mem(opus_ctx *c) {
    if (c->lproc_mem) return OPUS_OK;
    const size_t B = c->cfg.max_batch, N = c->cfg.max_new_tokens;
    const size_t o_st = align_up(sizeof(LogitsProcDesc)), o_gr = o_st + align_up(B * sizeof(int32_t)),
                 o_gp = o_gr + align_up(sizeof(GenOutDesc)), o_ls = o_gp + align_up(sizeof(GenOutDesc)),
                 o_rh = o_ls + align_up(B * sizeof(float));
    HIPC(hipMalloc((void **)&c->lproc_mem, o_rh + align_up(B * N * sizeof(float))));
    c->d_lproc = reinterpret_cast<LogitsProcDesc *>(c->lproc_mem);
    c->d_ridx = reinterpret_cast<int32_t *>(c->lproc_mem + o_st);
    c->d_lstep = c->d_ridx;                               // (opus_debug_logits_process only: no generate call in flight uses both)
    c->d_gen_raw = reinterpret_cast<GenOutDesc *>(c->lproc_mem + o_gr);
    c->d_gen_proc = reinterpret_cast<GenOutDesc *>(c->lproc_mem + o_gp);
    c->d_rlse = reinterpret_cast<float *>(c->lproc_mem + o_ls);
    c->d_rawh = reinterpret_cast<float *>(c->lproc_mem + o_rh);
    return OPUS_OK;
}

// guidance: keep = the call also needs the copy of the raw conditional rows
static int ensure_guid_mem(opus_ctx *c, bool keep) {
    const size_t B = c->cfg.max_batch;
    if (!c->guid_mem) {
        const size_t rows = align_up(2 * B * sizeof(float));
        const size_t o_ps = align_up(sizeof(float)), o_mx = o_ps + align_up(APART * B * sizeof(float)), o_lg = o_mx + rows,
                     o_ls = o_lg + rows;
        HIPC(hipMalloc((void **)&c->guid_mem, o_ls + rows));
        c->d_gscale = reinterpret_cast<float *>(c->guid_mem);
        c->d_gdpsum = reinterpret_cast<float *>(c->guid_mem + o_ps);
        c->d_gmax = reinterpret_cast<float *>(c->guid_mem + o_mx);
        c->d_glog = reinterpret_cast<float *>(c->guid_mem + o_lg);
        c->d_glse = reinterpret_cast<float *>(c->guid_mem + o_ls);
    }
    if (keep && !c->guid_keep) HIPC(hipMalloc((void **)&c->guid_keep, align_up((B / 2) * (size_t)c->cfg.dec_vocab * sizeof(float))));
    return OPUS_OK;
}

static int upload_guidance_scale(opus_ctx *c, float g, hipStream_t s) {
    int32_t w;
    memcpy(&w, &g, sizeof(w));
    HIPC(launch_upload_i32(&w, 1, reinterpret_cast<int32_t *>(c->d_gscale), s));
    return OPUS_OK;
}

// the setting's words through the kernel arguments (stream order, no host buffer outlives the call): the header and the used
// offsets, then the used ids
static int upload_lproc(opus_ctx *c, const LogitsProcDesc &h, hipStream_t s) {
    const int32_t *w = reinterpret_cast<const int32_t *>(&h);
    const int head = (int)(offsetof(LogitsProcDesc, bad_off) / sizeof(int32_t)) + h.n_bad + 1;
    int32_t *dw = reinterpret_cast<int32_t *>(c->d_lproc);
    HIPC(launch_upload_i32(w, head, dw, s));
    const int n_ids = h.bad_off[h.n_bad];
    const int o_ids = (int)(offsetof(LogitsProcDesc, bad_ids) / sizeof(int32_t));
    if (n_ids) HIPC(launch_upload_i32(w + o_ids, n_ids, dw + o_ids, s));
    return OPUS_OK;
}

static int upload_gen_desc(const GenOutDesc &h, GenOutDesc *d, hipStream_t s) {
    HIPC(launch_upload_i32(reinterpret_cast<const int32_t *>(&h), (int)(sizeof(GenOutDesc) / sizeof(int32_t)),
                           reinterpret_cast<int32_t *>(d), s));
    return OPUS_OK;
}

// next token per row: argmax (greedy) or temperature / top-p sampling, then the GenerationMixin bookkeeping.  With outputs asked for
// (opus_generate_scored): the first pass also sums the parts' exponentials and the step kernel writes the chosen token's
// log-probability (GEN_LOGPROBS), and / or the score writer copies the step's logits out (GEN_SCORES / GEN_LOGITS).
//
// Logits processors on (p.lproc): the processor kernel edits d_logits in place first, reading the history from d_out and the
// setting from d_lproc.  The raw outputs are taken before it: the raw logits (GEN_LOGITS, through the raw half of the split output
// descriptor) and the raw rows' log-sum-exp (GEN_LOGPROBS: one more pass over the logits); the kernel records the raw logit of every
// history position, where the step kernel finds the chosen token's raw logit if a penalty changed it.  The selection, the scores
// and the bookkeeping then run on the processed logits.
//
// Guidance on (p.guided): everything here works on the HB = rows / 2 conditional rows.  Behind the raw logits' copy and in front
// of the processors, one log-sum-exp pass over all rows and the combine (guidance.hip) overwrite row b with the guided
// scores of the pair (b, HB + b); the raw conditional log-sum-exp of that pass serves GEN_LOGPROBS, the chosen id's raw logit
// comes from the combine's copy of the raw rows.  Behind the step kernel, row HB + b is given row b's token.
static int select_next(opus_ctx *c, hipStream_t s, const StepPlan &p) {
    const int max_new = p.stride, n_eos = p.n_eos, pad_id = p.pad;
    int32_t *d_out = p.ids;
    c->phase = PH_DECODE;
    const opus_config &g = c->cfg;
    const int32_t *chosen = nullptr;
    const bool guid = p.guided;
    const int HB = guid ? p.rows / 2 : p.rows;      // rows the head works on
    const bool proc = p.lproc || p.cons || guid;    // the logits are edited in place: raw outputs first
    const bool lp = p.outs & GEN_LOGPROBS, sc = p.outs & (GEN_SCORES | GEN_LOGITS);
    const bool tl = p.outs & GEN_TOPLP;             // the k likeliest ids of the raw rows (topk.hip), k and the addresses from the descriptor
    const bool lse = lp || tl;                      // the raw rows' log-sum-exp is needed
    const size_t BV = (size_t)HB * g.dec_vocab;
    TopkArgs ta;
    ta.cand = c->d_tcand; ta.finished = c->d_fin; ta.step = c->d_step; ta.max_new = max_new;
    if (proc) {
        if (p.outs & GEN_LOGITS)
            KL(KC_OTHER, 8.0 * BV, launch_gen_scores(c->d_logits, HB, g.dec_vocab, c->d_gen_raw, c->d_step, max_new, 0.f, 1.f,
                                                     nullptr, nullptr, nullptr, s));
        if (guid) {
            KL(KC_GUIDANCE, 8.0 * BV, launch_guidance_lse_partial(c->d_logits, 2 * HB, g.dec_vocab, c->d_pval, c->d_gdpsum, s));
            KL(KC_GUIDANCE, 1024.0 * HB, launch_guidance_lse_final(c->d_pval, c->d_gdpsum, 2 * HB, c->d_gmax, c->d_glog, c->d_glse, s));
            if (tl) {
                ta.lse = c->d_glse; ta.desc = c->d_gen_raw;
                KL(KC_TOPK, 4.0 * BV, launch_topk_f32(c->d_logits, g.dec_vocab, HB, g.dec_vocab, ta, s));
            }
            KL(KC_GUIDANCE, (lp ? 16.0 : 12.0) * BV,
               launch_guidance_combine(c->d_logits, c->d_logits + BV, HB, g.dec_vocab, c->d_gmax, c->d_glog, c->d_gmax + HB,
                                       c->d_glog + HB, c->d_gscale, lp ? c->guid_keep : nullptr, s));
        } else if (lse) {
            KL(KC_OTHER, 4.0 * BV, launch_argmax_lse_partial(c->d_logits, HB, g.dec_vocab, c->d_pval, c->d_pidx, c->d_gpsum, s));
            KL(KC_OTHER, 512.0 * HB, launch_argmax_lse_final(c->d_pval, c->d_pidx, c->d_gpsum, HB, c->d_ridx, c->d_rlse, s));
            if (tl) {
                ta.lse = c->d_rlse; ta.desc = c->d_gen_raw;
                KL(KC_TOPK, 4.0 * BV, launch_topk_f32(c->d_logits, g.dec_vocab, HB, g.dec_vocab, ta, s));
            }
        }
        if (p.lproc)
            KL(KC_LOGITPROC, 12.0 * HB * max_new,
               launch_logits_proc(c->d_logits, HB, g.dec_vocab, d_out, max_new, c->d_step, max_new, c->d_eos, n_eos, c->d_lproc,
                                  lp && !guid ? c->d_rawh : nullptr, s));
        if (p.cons)                          // behind min_new_tokens, in front of the warpers (transformers' order)
            KL(KC_CONSTRAINT, 4.0 * BV,
               launch_token_constraint(c->d_logits, HB, g.dec_vocab, d_out, max_new, c->d_step, max_new, c->d_cons, s));
    }
    const bool warp = p.warp && p.temp > 0.f;       // the warpers narrow stage 2's threshold to a band and make the draw
    if (warp) {
        KL(KC_OTHER, 4.0 * 4 * HB * g.dec_vocab,
           launch_sample_select(c->d_logits, HB, g.dec_vocab, p.temp, p.top_p, p.top_k, nullptr, nullptr,
                                c->d_pval, c->d_pidx, c->d_probs, c->d_cand_i, c->d_cand_n, c->d_zpart, c->d_spart, nullptr, c->d_wlo,
                                lse && !proc ? c->d_gpsum : nullptr, nullptr, s));
        KL(KC_OTHER, 8.0 * HB * g.dec_vocab,
           launch_sample_warp_draw(HB, g.dec_vocab, c->d_warp, c->d_seed, c->d_step, c->d_probs, c->d_cand_i, c->d_cand_n, c->d_chosen,
                                   c->d_wlo, c->d_whi, s));
        chosen = c->d_chosen;
    } else if (p.temp > 0.f) {
        KL(KC_OTHER, 4.0 * 4 * HB * g.dec_vocab,
           launch_sample_select(c->d_logits, HB, g.dec_vocab, p.temp, p.top_p, p.top_k, c->d_seed, c->d_step,
                                c->d_pval, c->d_pidx, c->d_probs, c->d_cand_i, c->d_cand_n, c->d_zpart, c->d_spart, c->d_chosen, nullptr,
                                lse && !proc ? c->d_gpsum : nullptr, sc ? c->d_gthr : nullptr, s));
        chosen = c->d_chosen;
    } else if (lse && !proc) {
        KL(KC_OTHER, 4.0 * HB * g.dec_vocab,
           launch_argmax_lse_partial(c->d_logits, HB, g.dec_vocab, c->d_pval, c->d_pidx, c->d_gpsum, s));
    } else {
        KL(KC_OTHER, 4.0 * HB * g.dec_vocab, launch_argmax_partial(c->d_logits, HB, g.dec_vocab, c->d_pval, c->d_pidx, s));
    }
    if (tl && !proc) {                              // the plain path: the parts of the pass above give the lse, as in the step kernel
        ta.pval = c->d_pval; ta.psum = c->d_gpsum; ta.desc = c->d_gen;
        KL(KC_TOPK, 4.0 * BV, launch_topk_f32(c->d_logits, g.dec_vocab, HB, g.dec_vocab, ta, s));
    }
    if (proc ? (p.outs & GEN_SCORES) != 0 : sc)
        KL(KC_OTHER, 4.0 * HB * g.dec_vocab * (1 + ((p.outs & GEN_SCORES) ? 1 : 0) + ((p.outs & GEN_LOGITS) && !proc ? 1 : 0)),
           launch_gen_scores(c->d_logits, HB, g.dec_vocab, proc ? c->d_gen_proc : c->d_gen, c->d_step, max_new, p.temp,
                             p.top_p, c->d_pval, warp ? c->d_wlo : p.temp > 0.f ? c->d_gthr : nullptr, warp ? c->d_whi : nullptr, s));
    if (lp && proc)
        KL(KC_OTHER, 512.0 * HB + 8.0 * HB * max_new,
           launch_argmax_rawlp_step(c->d_pval, c->d_pidx, guid ? c->d_glse : c->d_rlse, p.lproc && !guid ? c->d_rawh : nullptr, chosen, HB, c->d_eos, n_eos, pad_id, c->d_fin, d_out,
                                    max_new, c->d_step, c->d_next, c->d_nunf, c->d_stop, p.n_stop, guid ? c->guid_keep : c->d_logits,
                                    g.dec_vocab, c->d_gen_proc, s));
    else if (lp)
        KL(KC_OTHER, 512.0 * HB + 8.0 * HB,
           launch_argmax_lse_step(c->d_pval, c->d_pidx, c->d_gpsum, chosen, HB, c->d_eos, n_eos, pad_id, c->d_fin, d_out, max_new,
                                  c->d_step, c->d_next, c->d_nunf, c->d_stop, p.n_stop, c->d_logits, g.dec_vocab, c->d_gen, s));
    else
        KL(KC_OTHER, 512.0 * HB,
           launch_argmax_step(c->d_pval, c->d_pidx, chosen, HB, c->d_eos, n_eos, pad_id, c->d_fin, d_out, max_new, c->d_step,
                              c->d_next, c->d_nunf, c->d_stop, p.n_stop, s));
    if (guid) KL(KC_GUIDANCE, 8.0 * HB, launch_guidance_pair_next(c->d_next, HB, s));
    return OPUS_OK;
}

// iteration body of the greedy loop: pick the next token from the current logits, then decode it.
static int greedy_body(opus_ctx *c, hipStream_t s, const StepPlan &p) {
    OPC(select_next(c, s, p));
    return decode_step(c, s, c->d_next);
}

// One step (greedy_body / stream_body) captured on s and instantiated into *exec.  The body's error wins over the capture's, a
// half-made graph is destroyed, and only an exec that exists is counted.
static int capture_step(opus_ctx *c, hipStream_t s, int (*body)(opus_ctx *, hipStream_t, const StepPlan &), const StepPlan &p,
                        hipGraphExec_t *exec) {
    hipGraph_t graph = nullptr;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = body(c, s, p);
    hipError_t ee = hipStreamEndCapture(s, &graph);
    if (rc != OPUS_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ee != hipSuccess) return fail(OPUS_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(ee));
    ee = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ee != hipSuccess) { *exec = nullptr; return fail(OPUS_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(ee)); }
    ++c->graph_instantiations;
    return OPUS_OK;
}

// What opus_generate_* and opus_stream_begin do alike in front of their prefill, under the caller's name: the checks of the
// sampling settings, the token budget and the EOS list, the uploads of the EOS ids and the seed, the clears of the rows' finished
// flags and of the steps' unfinished counts.  (seed: the caller's own word, the source of an asynchronous copy.)
static int begin_generation(opus_ctx *c, const char *who, float temperature, float top_p, int32_t max_new, const int32_t *eos_ids,
                            int32_t n_eos, const uint64_t *seed, int rows, int steps, hipStream_t s) {
    if (temperature < 0.f || top_p <= 0.f || top_p > 1.f) return fail(OPUS_EBADARG, "%s: temperature >= 0 and 0 < top_p <= 1", who);
    if (max_new < 1 || max_new > c->cfg.max_new_tokens)
        return fail(OPUS_ESHAPE, "%s: max_new=%d exceeds max_new_tokens=%d", who, max_new, c->cfg.max_new_tokens);
    if (n_eos < 0 || n_eos > 64 || (n_eos > 0 && !eos_ids)) return fail(OPUS_EBADARG, "%s: eos list", who);
    if (n_eos) HIPC(hipMemcpyAsync(c->d_eos, eos_ids, n_eos * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c->d_seed, seed, sizeof(*seed), hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(c->d_fin, 0, rows * sizeof(int32_t), s));
    HIPC(hipMemsetAsync(c->d_nunf, 0, (size_t)steps * sizeof(int32_t), s));
    return OPUS_OK;
}

// TokenConstraintDesc::start_div of the device descriptor (uploaded only when it changes: the plain call launches nothing here)
static int set_cons_start_div(opus_ctx *c, int32_t div, hipStream_t s) {
    if (div == c->cons_start_div) return OPUS_OK;
    int32_t *w = reinterpret_cast<int32_t *>(c->d_cons) + offsetof(TokenConstraintDesc, start_div) / sizeof(int32_t);
    HIPC(launch_upload_i32(&div, 1, w, s));
    c->cons_start_div = div;
    return OPUS_OK;
}

static int generate_impl(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                         const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature, float top_p, uint64_t seed,
                         int32_t *d_out_ids, int32_t *n_out, void *stream, const GenOutDesc *outs = nullptr, int32_t nret = 1,
                         const BehindArgs *behind = nullptr, const float *guidance = nullptr) {
    GenOutDesc with_top{};                   // the scored calls under opus_set_gen_top_logprobs: their outputs + the setter's
    if (outs && c && c->top_k > 0) {
        with_top = *outs;
        with_top.top_lp = c->top_lp; with_top.top_ids = c->top_ids; with_top.top_k = c->top_k;
        outs = &with_top;
    }
    // guidance (opus_generate_scored_guided; nret 1, no behind): B = 2 P rows, the head of every step works on the first P
    // behind (opus_generate_scored_behind): the B rows are suffixes of T right-padded positions behind a detached prefix (no mask)
    OPC(need_ready(c));
    if (!behind) OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    else if (B < 1 || B > c->cfg.max_batch) return fail(OPUS_ESHAPE, "generate: B=%d decoder rows, the context holds max_batch=%d", B, c->cfg.max_batch);
    OPC(check_fanout(c, B, nret, "generate"));
    const int32_t BN = B * nret;             // decoder rows: the loop, its buffers and the captured step are those of a BN-row batch
    if (!d_out_ids || !n_out) return fail(OPUS_EBADARG, "generate_greedy: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const opus_config &g = c->cfg;
    OPC(begin_generation(c, "generate_greedy", temperature, top_p, max_new, eos_ids, n_eos, &seed, BN, max_new, s));
    StepPlan plan;
    plan.rows = BN; plan.guided = guidance != nullptr; plan.stride = max_new; plan.ids = d_out_ids; plan.n_eos = n_eos; plan.pad = pad_id;
    plan.temp = temperature; plan.top_p = top_p; plan.top_k = c->samp_top_k; plan.n_stop = c->n_stop;
    plan.lproc = c->lproc_on; plan.cons = c->cons_on; plan.warp = temperature > 0.f && c->warp_on();
    if (plan.warp) OPC(upload_warpers(c, s));
    if (outs) plan.outs = (outs->token_lp ? GEN_LOGPROBS : 0) | (outs->scores ? GEN_SCORES : 0) | (outs->logits ? GEN_LOGITS : 0) |
                          (outs->top_k > 0 ? GEN_TOPLP : 0);
    if (plan.outs & GEN_TOPLP) OPC(ensure_topk_mem(c));
    if (plan.outs) {
        OPC(ensure_gen_mem(c));
        c->h_gen = *outs;                    // (a member: the source outlives the asynchronous copy)
        HIPC(hipMemcpyAsync(c->d_gen, &c->h_gen, sizeof(GenOutDesc), hipMemcpyHostToDevice, s));
    }
    const int32_t HB = guidance ? B / 2 : B;                // rows (before the fan-out) with a state of their own
    if (c->cons_on && c->cons_n_start != 1 && c->cons_n_start != HB)
        return fail(OPUS_ESHAPE, "generate: the token constraint has %d per-row start states, the batch %d rows", c->cons_n_start, HB);
    if (c->cons_on) OPC(set_cons_start_div(c, nret, s));    // one start state per prompt: decoder row r starts at start[r / nret]
    if (guidance) {
        OPC(ensure_guid_mem(c, (plan.outs & GEN_LOGPROBS) != 0));
        OPC(upload_guidance_scale(c, *guidance, s));
    }
    if (c->lproc_on || c->cons_on || guidance) {
        if (c->lproc_on && max_new > LP_MAX_HIST)
            return fail(OPUS_ESHAPE, "generate: logits processors keep a history of at most %d ids (max_new=%d)", LP_MAX_HIST, max_new);
        OPC(ensure_lproc_mem(c));
        if (c->lproc_on) OPC(upload_lproc(c, c->h_lproc, s));
        if (plan.outs) {                     // raw logits before the processors, the rest after them
            OPC(upload_gen_desc(GenOutDesc{nullptr, nullptr, outs->logits, outs->top_lp, outs->top_ids, outs->top_k, 0}, c->d_gen_raw, s));
            OPC(upload_gen_desc(GenOutDesc{outs->token_lp, outs->scores, nullptr, nullptr}, c->d_gen_proc, s));
        }
    }
    if (behind) OPC(prefill_behind(c, s, *behind, (const half_t *)d_embeds, B, T));
    else OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T, false, nullptr, nret));

    // OPUS_NO_GRAPH=1: eager launches (rocprofv3 --pmc cannot collect counters through graph replays)
    const bool use_graph = s != nullptr && !c->timing && !getenv("OPUS_NO_GRAPH");
    opus_ctx::GraphEntry *ge = nullptr;
    if (use_graph)
        for (auto &e : c->graphs)
            if (e.exec && same_step(e.key, plan)) { ge = &e; break; }
    const bool same_graph = ge != nullptr;
    std::vector<int32_t> nunf(max_new, 1);
    int produced = 0;
    for (int i = 0; i < max_new; ++i) {
        if (i + 1 == max_new) {   // last token: no decode behind it
            OPC(select_next(c, s, plan));
            produced = i + 1;
            break;
        }
        ++c->decode_steps;
        if (!use_graph || (i == 0 && !same_graph)) {
            OPC(greedy_body(c, s, plan));    // eager (also warms lazily-set attributes)
        } else {
            if (!ge) {
                opus_ctx::GraphEntry e;
                OPC(capture_step(c, s, greedy_body, plan, &e.exec));
                e.key = plan;
                if ((int)c->graphs.size() >= opus_ctx::MAX_GRAPHS) {           // least recently used out
                    size_t v = 0;
                    for (size_t k = 1; k < c->graphs.size(); ++k) if (c->graphs[k].used < c->graphs[v].used) v = k;
                    (void)hipGraphExecDestroy(c->graphs[v].exec);
                    c->graphs.erase(c->graphs.begin() + v);
                }
                c->graphs.push_back(e);
                ge = &c->graphs.back();
            }
            ge->used = ++c->graph_clock;
            ++c->graph_replays;
            HIPC(hipGraphLaunch(ge->exec, s));
        }
        produced = i + 1;
        // HF stops as soon as every row has finished.  The host runs ahead of the GPU, so it polls with a BOUNDED run-ahead instead
        // of a synchronisation per step: step i's unfinished count is copied to pinned memory behind an event, and before step
        // i + 1 is enqueued the host waits for step i - 2's event (the GPU still has a step queued: no bubble) and stops when that
        // count is zero - at most 2 steps are decoded past the last row's EOS (rounds 1-4: a stream synchronisation every 8 steps,
        // up to 7 wasted steps).  Finished rows emit pad, so the ids are identical and n_out is computed exactly below.
        if (n_eos > 0 || plan.n_stop > 0) {
            HIPC(hipMemcpyAsync(c->h_nunf + i, c->d_nunf + i, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPC(hipEventRecord(c->poll_ev[i % opus_ctx::POLL_RING], s));
            if (i >= opus_ctx::POLL_LAG) {
                HIPC(hipEventSynchronize(c->poll_ev[(i - opus_ctx::POLL_LAG) % opus_ctx::POLL_RING]));
                if (c->h_nunf[i - opus_ctx::POLL_LAG] == 0) break;
            }
        }
    }
    HIPC(hipMemcpyAsync(nunf.data(), c->d_nunf, (size_t)produced * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OPC(handoff_check(c, s));                                         // (synchronises the stream)
    int n = produced;
    for (int k = 0; k < produced; ++k) if (nunf[k] == 0) { n = k + 1; break; }
    *n_out = n;
    return OPUS_OK;
}

// Opt-in early stop on a token sequence ("### early-stop as an opt-in").  The reference decodes to
// max_new_tokens and cuts the TEXT at the first "###" afterwards (eval/run_opus_ddp.py:19-27); with the ids of "###" set
// here a row is finished as soon as its new ids end with them (later positions hold pad_id, as after an EOS), which leaves
// the cut text unchanged and lets a batch stop early.  n = 0 clears it.  Host ids, at most 8.
extern "C" int opus_set_stop_sequence(opus_ctx *c, const int32_t *ids, int32_t n) {
    if (!c || n < 0 || n > 8 || (n > 0 && !ids)) return fail(OPUS_EBADARG, "set_stop_sequence: 0 <= n <= 8 ids");
    HIPC(hipSetDevice(c->device));
    if (n) HIPC(hipMemcpy(c->d_stop, ids, n * sizeof(int32_t), hipMemcpyHostToDevice));
    c->n_stop = n;
    drop_graphs(c);                                                               // the captured step holds n_stop
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ continuous batching
// One live decode batch (a session) whose done rows are handed to new prompts: opus_stream_begin prefills the first rows,
// opus_stream_run decodes until enough rows are done, opus_stream_refill places new prompts (prefilled elsewhere, a detached
// snapshot + their last-position logits) under done rows, opus_stream_end closes the session.  Step t of a session writes column t
// of the id buffer [B, S] (S = max_new_tokens of the context, the session's step budget) and cache slot T0 + t; a row's occupant
// began at start[r].  The host looks at the rows' state STREAM_LAG steps behind what it enqueues (the event ring of generate_impl),
// so a boundary's decision is a function of the rows' end steps only, never of how far the GPU happens to be.
static int ensure_stream_mem(opus_ctx *c) {
    if (c->stream_mem) return OPUS_OK;
    const size_t B = c->cfg.max_batch;
    const size_t words = 2 * B + 1 + 5 * B + 2;            // start | poll | nks, rows, src, off [B + 2], list (one upload)
    HIPC(hipMalloc((void **)&c->stream_mem, words * sizeof(int32_t)));
    HIPC(hipHostMalloc((void **)&c->h_poll, opus_ctx::STREAM_RING * (B + 1) * sizeof(int32_t), hipHostMallocDefault));
    int32_t *w = reinterpret_cast<int32_t *>(c->stream_mem);
    c->d_sstart = w;
    c->d_spoll = w + B;
    c->d_snks = w + 2 * B + 1;
    c->d_srows = c->d_snks + B;
    c->d_ssrc = c->d_srows + B;
    c->d_soff = c->d_ssrc + B;
    c->d_slist = c->d_soff + B + 2;
    return OPUS_OK;
}

// one step of a session: the head of generate's step, the rows' budgets and end steps, the decode of the chosen tokens
static int stream_body(opus_ctx *c, hipStream_t s, const StepPlan &p) {
    OPC(select_next(c, s, p));
    KL(KC_OTHER, 16.0 * p.rows, launch_stream_finish(c->d_step, c->d_sstart, c->d_fin, c->d_spoll, p.rows, p.budget, s));
    return decode_step(c, s, c->d_next);
}

extern "C" int32_t opus_stream_lag(void) { return opus_ctx::STREAM_LAG; }

extern "C" int opus_stream_begin(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                                 const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature, float top_p, uint64_t seed,
                                 int32_t *d_ids, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    if (!d_ids) return fail(OPUS_EBADARG, "stream_begin: null pointer");
    const opus_config &g = c->cfg;
    if (c->lproc_on || c->cons_on)
        return fail(OPUS_EUNSUPPORTED, "stream_begin: logits processors and token constraints count steps from 0 for every row: not "
                                       "built for rows that begin at a later step");
    OPC(ensure_stream_mem(c));
    hipStream_t s = (hipStream_t)stream;
    OPC(begin_generation(c, "stream_begin", temperature, top_p, max_new, eos_ids, n_eos, &seed, B, g.max_new_tokens, s));
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T));
    c->phase = PH_DECODE;
    KL(KC_OTHER, 8.0 * B, launch_stream_reset(c->d_sstart, c->d_spoll, B, s));
    opus_ctx::StreamState &st = c->st;
    st.T0 = T; st.t = 0;
    st.plan = StepPlan();
    st.plan.rows = B; st.plan.stride = g.max_new_tokens; st.plan.ids = d_ids; st.plan.n_eos = n_eos; st.plan.pad = pad_id;
    st.plan.temp = temperature; st.plan.top_p = top_p; st.plan.top_k = c->samp_top_k; st.plan.n_stop = c->n_stop;
    st.plan.budget = max_new;
    st.plan.warp = temperature > 0.f && c->warp_on();
    if (st.plan.warp) OPC(upload_warpers(c, s));
    st.start.assign(B, 0);
    st.on = true;
    return OPUS_OK;
}

extern "C" int opus_stream_run(opus_ctx *c, int32_t t_min, int32_t min_free, int32_t t_max, int32_t *t_out, int32_t *h_end,
                               void *stream) {
    if (!c || !t_out || !h_end) return fail(OPUS_EBADARG, "stream_run: null pointer");
    HIPC(hipSetDevice(c->device));
    opus_ctx::StreamState &st = c->st;
    if (!st.on) return fail(OPUS_ESTATE, "stream_run: no session is open (opus_stream_begin; a prefill on this context ends one)");
    hipStream_t s = (hipStream_t)stream;
    const int B = st.plan.rows, S = c->cfg.max_new_tokens;
    constexpr int LAG = opus_ctx::STREAM_LAG, RING = opus_ctx::STREAM_RING;
    if (t_max > S) t_max = S;
    if (min_free < 1) min_free = 1;
    const bool use_graph = s != nullptr && !c->timing && !getenv("OPUS_NO_GRAPH");
    opus_ctx::GraphEntry &ge = c->stream_graph;
    if (ge.exec && !same_step(ge.key, st.plan)) {
        (void)hipGraphExecDestroy(ge.exec);
        ge = opus_ctx::GraphEntry();
    }
    for (;;) {                                                      // (at most S + 1 boundaries: t grows by one per round)
        const int t = st.t, sv = t - LAG;
        int ndone = 0;
        for (int r = 0; r < B; ++r) h_end[r] = -1;
        if (sv >= 0) {
            HIPC(hipEventSynchronize(c->poll_ev[sv % RING]));
            const int32_t *p = c->h_poll + (size_t)(sv % RING) * (c->cfg.max_batch + 1);
            for (int r = 0; r < B; ++r)
                if (st.start[r] <= sv && p[r] >= 0) {               // (an earlier occupant's end step is not this row's)
                    h_end[r] = p[r];
                    ++ndone;
                }
        }
        if (ndone == B || t >= t_max || (t >= t_min && ndone >= min_free)) {
            *t_out = t;
            return OPUS_OK;
        }
        if (!use_graph || (!ge.exec && t == 0)) {
            OPC(stream_body(c, s, st.plan));                        // eager (the first step also warms lazily-set attributes)
        } else {
            if (!ge.exec) {
                OPC(capture_step(c, s, stream_body, st.plan, &ge.exec));
                ge.key = st.plan;
            }
            ++c->graph_replays;
            HIPC(hipGraphLaunch(ge.exec, s));
        }
        HIPC(hipMemcpyAsync(c->h_poll + (size_t)(t % RING) * (c->cfg.max_batch + 1), c->d_spoll, (size_t)(B + 1) * sizeof(int32_t),
                            hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(c->poll_ev[t % RING], s));
        ++st.t;
        ++c->decode_steps;
        ++c->stream_steps;
    }
}

extern "C" int opus_stream_refill(opus_ctx *c, const opus_prefix_snap *snap, int32_t n, const int32_t *h_rows, const int32_t *h_src,
                                  const float *d_last_logits, const int32_t *h_len, void *stream) {
    OPC(need_ready(c));
    opus_ctx::StreamState &st = c->st;
    if (!st.on) return fail(OPUS_ESTATE, "stream_refill: no session is open");
    if (!h_rows || !h_src || !d_last_logits || !h_len) return fail(OPUS_EBADARG, "stream_refill: null pointer");
    const opus_config &g = c->cfg;
    const int B = st.plan.rows, MB = g.max_batch, S = g.max_new_tokens, t = st.t, L = st.T0 + t;
    PrefixSrc ps;
    OPC(resolve_prefix(c, "stream_refill", snap, 0, 0, ps));
    if (n < 1 || n > B) return fail(OPUS_ESHAPE, "stream_refill: %d rows listed, the session has %d", n, B);
    if (t + st.plan.budget > S)
        return fail(OPUS_ESHAPE, "stream_refill: a row that begins at step %d cannot end inside the session's %d steps (budget %d)", t, S,
                    st.plan.budget);
    if (d_last_logits == c->d_logits) return fail(OPUS_EBADARG, "stream_refill: the logits rows must come from another buffer");
    std::vector<int32_t> w(5 * (size_t)MB + 2, 0), seen(B, 0);
    int32_t *nks = w.data(), *rows = nks + MB, *src = rows + MB, *off = src + MB, *list = off + MB + 2;
    for (int i = 0; i < n; ++i) {
        const int r = h_rows[i], p = h_src[i];
        if (r < 0 || r >= B || seen[r]) return fail(OPUS_EBADARG, "stream_refill: row %d outside [0, %d) or listed twice", r, B);
        if (p < 0 || p >= ps.P) return fail(OPUS_EBADARG, "stream_refill: snapshot row %d of row %d outside [0, %d)", p, r, ps.P);
        const int len = ps.Tp - ps.kst[p];
        if (h_len[i] != len) return fail(OPUS_EBADARG, "stream_refill: row %d: length %d, the snapshot row holds %d slots", r, h_len[i], len);
        if (len < 1 || len > L) return fail(OPUS_ESHAPE, "stream_refill: a prompt of %d slots does not fit under %d slots", len, L);
        seen[r] = 1;
        nks[r] = L - len;
        rows[i] = r;
        src[i] = p;
    }
    int k = 0;
    for (int p = 0; p < ps.P; ++p) {                                // kv_place's grouping: the listed rows of every snapshot row
        off[p] = k;
        for (int i = 0; i < n; ++i)
            if (h_src[i] == p) list[k++] = h_rows[i];
    }
    off[ps.P] = k;
    hipStream_t s = (hipStream_t)stream;
    new_epoch(c);                                                   // (prefix handles of this context are stale)
    st.on = true;
    c->h_kstart.clear();
    c->phase = PH_OTHER;
    HIPC(launch_upload_i32(w.data(), (int)w.size(), c->d_snks, s));
    KvPlaceParams kp;
    kp.snap_k = reinterpret_cast<const half_t *>(snap->d_k); kp.snap_v = reinterpret_cast<const half_t *>(snap->d_v);
    kp.kstart = snap->d_kstart; kp.P = ps.P; kp.Tp = ps.Tp; kp.kc = c->kc; kp.vc = c->vc;
    kp.cache_sl = c->cache_sl; kp.cache_sb = c->cache_sb; kp.cache_sh = c->cache_sh;
    kp.list = c->d_slist; kp.off = c->d_soff; kp.new_kstart = c->d_snks;
    kp.layers = g.dec_layers; kp.nkv = g.dec_kv_heads; kp.hd = g.dec_head_dim;
    double slots = 0.0;
    for (int i = 0; i < n; ++i) slots += h_len[i];
    KL(KC_OTHER, 2.0 * slots * 2.0 * g.dec_layers * g.dec_kv_heads * g.dec_head_dim * sizeof(half_t), launch_kv_place(kp, s));
    KL(KC_OTHER, 8.0 * n * g.dec_vocab,
       launch_stream_refill(c->d_srows, c->d_ssrc, c->d_snks, n, d_last_logits, c->d_logits, g.dec_vocab, c->d_kstart, c->d_sstart,
                            c->d_fin, c->d_spoll, st.plan.ids, S, t, s));
    for (int i = 0; i < n; ++i) st.start[h_rows[i]] = t;
    ++c->stream_refills;
    return OPUS_OK;
}

extern "C" int opus_stream_end(opus_ctx *c, int32_t *h_end, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    HIPC(hipSetDevice(c->device));
    if (!c->st.on) return fail(OPUS_ESTATE, "stream_end: no session is open");
    c->st.on = false;
    hipStream_t s = (hipStream_t)stream;
    // the rows' end steps with every enqueued step complete (no lag: nothing is decided from them but what to harvest)
    if (h_end) HIPC(hipMemcpyAsync(h_end, c->d_spoll, (size_t)c->st.plan.rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return handoff_check(c, s);                                     // (synchronises the stream)
}

// Test support: synchronises `stream` and copies the session's row words to the host - kstart, the finished flags, start and the
// end steps [rows of the session each] - and the cache epoch.  poison != 0 first fills the whole KV cache with that byte.
extern "C" int opus_debug_stream_state(opus_ctx *c, int32_t *h_kstart, int32_t *h_fin, int32_t *h_start, int32_t *h_end, int64_t *epoch,
                                       int32_t poison, void *stream) {
    if (!c || !h_kstart || !h_fin || !h_start || !h_end || !epoch) return fail(OPUS_EBADARG, "debug_stream_state: null pointer");
    HIPC(hipSetDevice(c->device));
    if (!c->st.on) return fail(OPUS_ESTATE, "debug_stream_state: no session is open");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = c->st.plan.rows, cache = (size_t)c->cache_sl * c->cfg.dec_layers * sizeof(half_t);
    if (poison) {
        HIPC(hipMemsetAsync(c->kc, poison & 255, cache, s));
        HIPC(hipMemsetAsync(c->vc, poison & 255, cache, s));
    }
    HIPC(hipMemcpyAsync(h_kstart, c->d_kstart, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h_fin, c->d_fin, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h_start, c->d_sstart, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h_end, c->d_spoll, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    *epoch = c->epoch;
    return OPUS_OK;
}

// A logits-processor setting from host values (opus_set_logits_processors / opus_debug_logits_process): checked against the
// capacities; V > 0 also bounds the ids.
static int make_lproc(LogitsProcDesc &d, float penalty, int32_t ngram, int32_t min_new, const int32_t *bad_ids, const int32_t *bad_off,
                      int32_t n_bad, int V, const char *who) {
    if (!(penalty > 0.f) || !(penalty < INFINITY)) return fail(OPUS_EBADARG, "%s: repetition_penalty must be a positive float", who);
    if (ngram < 0) return fail(OPUS_EBADARG, "%s: no_repeat_ngram_size must be >= 0", who);
    if (min_new < 0) return fail(OPUS_EBADARG, "%s: min_new_tokens must be >= 0", who);
    if (n_bad < 0 || n_bad > LP_MAX_BAD) return fail(OPUS_EBADARG, "%s: %d bad-word entries (at most %d)", who, n_bad, LP_MAX_BAD);
    if (n_bad > 0 && (!bad_ids || !bad_off)) return fail(OPUS_EBADARG, "%s: null bad-word table", who);
    if (n_bad > 0 && bad_off[0] != 0) return fail(OPUS_EBADARG, "%s: bad_offsets[0] must be 0", who);
    for (int e = 0; e < n_bad; ++e) {
        const int L = bad_off[e + 1] - bad_off[e];
        if (L < 1 || L > LP_MAX_BAD_LEN) return fail(OPUS_EBADARG, "%s: bad-word entry %d has %d ids (1 to %d)", who, e, L, LP_MAX_BAD_LEN);
    }
    const int n_ids = n_bad > 0 ? bad_off[n_bad] : 0;
    if (n_ids > LP_MAX_BAD_IDS) return fail(OPUS_EBADARG, "%s: %d bad-word ids (at most %d in all)", who, n_ids, LP_MAX_BAD_IDS);
    for (int i = 0; i < n_ids; ++i)
        if (bad_ids[i] < 0 || (V > 0 && bad_ids[i] >= V)) return fail(OPUS_EBADARG, "%s: bad-word id %d outside [0, %d)", who, bad_ids[i], V);
    d = LogitsProcDesc{penalty, ngram, min_new, n_bad, {}, {}};
    for (int e = 0; e <= n_bad; ++e) d.bad_off[e] = n_bad > 0 ? bad_off[e] : 0;
    for (int i = 0; i < n_ids; ++i) d.bad_ids[i] = bad_ids[i];
    return OPUS_OK;
}

// generate()'s logits processors for the calls that follow (see include/opus_pllm.h).  Only "on / off" enters the captured step's
// identity: the values travel in the device descriptor every call uploads, so a new penalty needs no new graph.
extern "C" int opus_set_logits_processors(opus_ctx *c, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_new_tokens,
                                          const int32_t *bad_ids, const int32_t *bad_offsets, int32_t n_bad) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    LogitsProcDesc d;
    OPC(make_lproc(d, repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_ids, bad_offsets, n_bad, c->cfg.dec_vocab,
                   "set_logits_processors"));
    c->h_lproc = d;
    c->lproc_on = d.penalty != 1.0f || d.ngram > 0 || d.min_new > 0 || d.n_bad > 0;
    return OPUS_OK;
}

/* Diagnostic: the processor kernel alone on caller memory - fp32 logits [B, V] edited in place, history d_hist [B, hist_stride]
   of hist_len ids per row, host EOS ids, the setting as opus_set_logits_processors takes it. */
extern "C" int opus_debug_logits_process(opus_ctx *c, float *d_logits, int32_t B, int32_t V, const int32_t *d_hist, int32_t hist_stride,
                                         int32_t hist_len, const int32_t *eos_ids, int32_t n_eos, float repetition_penalty,
                                         int32_t no_repeat_ngram_size, int32_t min_new_tokens, const int32_t *bad_ids,
                                         const int32_t *bad_offsets, int32_t n_bad, void *stream) {
    if (!c || !d_logits || (hist_len > 0 && !d_hist) || (n_eos > 0 && !eos_ids)) return fail(OPUS_EBADARG, "debug_logits_process: null pointer");
    if (B < 1 || V < 1 || hist_len < 0 || hist_len > LP_MAX_HIST || hist_stride < hist_len || n_eos < 0 || n_eos > 64)
        return fail(OPUS_ESHAPE, "debug_logits_process: B=%d V=%d history %d (stride %d, at most %d) n_eos=%d", B, V, hist_len,
                    hist_stride, LP_MAX_HIST, n_eos);
    LogitsProcDesc d;
    OPC(make_lproc(d, repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_ids, bad_offsets, n_bad, V, "debug_logits_process"));
    HIPC(hipSetDevice(c->device));
    OPC(ensure_lproc_mem(c));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    OPC(upload_lproc(c, d, s));
    if (n_eos) HIPC(launch_upload_i32(eos_ids, n_eos, c->d_eos, s));
    HIPC(launch_upload_i32(&hist_len, 1, c->d_lstep, s));
    KL(KC_LOGITPROC, 12.0 * B * hist_len, launch_logits_proc(d_logits, B, V, d_hist, hist_stride, c->d_lstep, hist_len, c->d_eos, n_eos,
                                                             c->d_lproc, nullptr, s));
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ constrained decoding
static int ensure_cons_mem(opus_ctx *c) {
    if (c->cons_mem) return OPUS_OK;
    const size_t o_st = align_up(sizeof(TokenConstraintDesc)), o_sp = o_st + align_up(2 * (size_t)c->cfg.max_batch * sizeof(int32_t));
    HIPC(hipMalloc((void **)&c->cons_mem, o_sp + align_up(sizeof(int32_t))));
    c->d_cons = reinterpret_cast<TokenConstraintDesc *>(c->cons_mem);
    c->d_cstate = reinterpret_cast<int32_t *>(c->cons_mem + o_st);
    c->d_cstep = reinterpret_cast<int32_t *>(c->cons_mem + o_sp);
    return OPUS_OK;
}

// The token automaton generate() is constrained to, for the calls of this context that follow (see include/opus_pllm.h).  The
// table is checked on the host, then copied to a device allocation the context owns; only "on / off" enters the captured step's
// identity - the table's addresses and sizes travel in a device descriptor, so another table needs no new graph.
extern "C" int opus_set_token_constraint(opus_ctx *c, int32_t n_states, const int32_t *edge_off, const int32_t *edge_tok,
                                         const int32_t *edge_next, int32_t n_edges, const uint8_t *completing, const int32_t *end_ids,
                                         int32_t n_end, const int32_t *start, int32_t n_start, void *stream) {
    const char *who = "set_token_constraint";
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (n_states == 0) {                     // off (the table stays allocated for the next one)
        c->cons_on = false;
        return OPUS_OK;
    }
    const int V = c->cfg.dec_vocab;
    if (n_states < 1 || n_edges < 0 || !edge_off || !completing || !end_ids || !start || (n_edges > 0 && (!edge_tok || !edge_next)))
        return fail(OPUS_EBADARG, "%s: null table or negative size", who);
    if (n_end < 1 || n_end > TC_MAX_END) return fail(OPUS_EBADARG, "%s: %d end ids (1 to %d)", who, n_end, TC_MAX_END);
    if (n_start < 1 || n_start > c->cfg.max_batch)
        return fail(OPUS_EBADARG, "%s: %d start states (1, or one per row up to max_batch=%d)", who, n_start, c->cfg.max_batch);
    if (V > TC_MAX_VOCAB) return fail(OPUS_ESHAPE, "%s: vocabulary %d above the kernel's %d", who, V, TC_MAX_VOCAB);
    if (edge_off[0] != 0 || edge_off[n_states] != n_edges) return fail(OPUS_EBADARG, "%s: edge_off must run from 0 to n_edges", who);
    if (edge_off[1] != 0 || !completing[0]) return fail(OPUS_EBADARG, "%s: state 0 is the end state (no edges, completing)", who);
    int32_t max_id = -1;
    for (int s = 0; s < n_states; ++s) {
        const int e0 = edge_off[s], e1 = edge_off[s + 1];
        if (e1 < e0 || e1 > n_edges) return fail(OPUS_EBADARG, "%s: edge_off not monotone at state %d", who, s);
        for (int e = e0; e < e1; ++e) {
            if (edge_tok[e] < 0 || edge_tok[e] >= V) return fail(OPUS_EBADARG, "%s: id %d outside [0, %d)", who, edge_tok[e], V);
            if (e > e0 && edge_tok[e] <= edge_tok[e - 1]) return fail(OPUS_EBADARG, "%s: ids of state %d not ascending", who, s);
            if (edge_next[e] < 0 || edge_next[e] >= n_states) return fail(OPUS_EBADARG, "%s: target %d outside [0, %d)", who, edge_next[e], n_states);
        }
        if (e1 > e0 && edge_tok[e1 - 1] > max_id) max_id = edge_tok[e1 - 1];
        if (e1 == e0 && !completing[s]) return fail(OPUS_EBADARG, "%s: state %d allows nothing", who, s);
    }
    for (int k = 0; k < n_end; ++k) {
        if (end_ids[k] < 0 || end_ids[k] >= V) return fail(OPUS_EBADARG, "%s: end id %d outside [0, %d)", who, end_ids[k], V);
        if (end_ids[k] > max_id) max_id = end_ids[k];
    }
    for (int k = 0; k < n_start; ++k)
        if (start[k] < 0 || start[k] >= n_states) return fail(OPUS_EBADARG, "%s: start state %d outside [0, %d)", who, start[k], n_states);

    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    OPC(ensure_cons_mem(c));
    const size_t o_tok = align_up((size_t)(n_states + 1) * 4), o_nxt = o_tok + align_up((size_t)n_edges * 4),
                 o_end = o_nxt + align_up((size_t)n_edges * 4), o_sta = o_end + align_up((size_t)n_end * 4),
                 o_cmp = o_sta + align_up((size_t)n_start * 4), total = o_cmp + align_up((size_t)n_states);
    HIPC(hipStreamSynchronize(s));           // a call in flight may still read the table that is replaced
    if (total > c->cons_tab_bytes) {
        if (c->cons_tab) HIPC(hipFree(c->cons_tab));
        c->cons_tab = nullptr;
        c->cons_tab_bytes = 0;
        c->cons_on = false;
        HIPC(hipMalloc((void **)&c->cons_tab, total));
        c->cons_tab_bytes = total;
    }
    char *t = c->cons_tab;
    HIPC(hipMemcpyAsync(t, edge_off, (size_t)(n_states + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_edges) {
        HIPC(hipMemcpyAsync(t + o_tok, edge_tok, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(t + o_nxt, edge_next, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    }
    HIPC(hipMemcpyAsync(t + o_end, end_ids, (size_t)n_end * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_sta, start, (size_t)n_start * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_cmp, completing, (size_t)n_states, hipMemcpyHostToDevice, s));
    TokenConstraintDesc h{};
    h.edge_off = reinterpret_cast<const int32_t *>(t);
    h.edge_tok = reinterpret_cast<const int32_t *>(t + o_tok);
    h.edge_next = reinterpret_cast<const int32_t *>(t + o_nxt);
    h.completing = reinterpret_cast<const uint8_t *>(t + o_cmp);
    h.end_ids = reinterpret_cast<const int32_t *>(t + o_end);
    h.start = reinterpret_cast<const int32_t *>(t + o_sta);
    h.state = c->d_cstate;
    h.n_states = n_states; h.n_end = n_end; h.n_start = n_start; h.state_stride = c->cfg.max_batch;
    h.start_div = 1;
    HIPC(launch_upload_i32(reinterpret_cast<const int32_t *>(&h), (int)(sizeof(h) / sizeof(int32_t)),
                           reinterpret_cast<int32_t *>(c->d_cons), s));
    HIPC(hipStreamSynchronize(s));           // the host arrays are the caller's again
    c->cons_n_start = n_start;
    c->cons_start_div = 1;
    c->cons_max_id = max_id;
    c->cons_on = true;
    return OPUS_OK;
}

/* Diagnostic: the constraint kernel alone on caller memory - fp32 logits [B, V] masked in place for rows whose history is
   d_hist[b * hist_stride + 0 .. hist_len), against the table of the last opus_set_token_constraint.  The state words are
   brought to the history's end by the product kernel's own transition, one launch per id (the kernel never walks a history),
   and copied to d_state_out [B] (optional). */
extern "C" int opus_debug_token_constraint(opus_ctx *c, float *d_logits, int32_t B, int32_t V, const int32_t *d_hist,
                                           int32_t hist_stride, int32_t hist_len, int32_t *d_state_out, void *stream) {
    if (!c || !d_logits || (hist_len > 0 && !d_hist)) return fail(OPUS_EBADARG, "debug_token_constraint: null pointer");
    if (!c->cons_on) return fail(OPUS_ESTATE, "debug_token_constraint: no table set (opus_set_token_constraint)");
    if (B < 1 || B > c->cfg.max_batch || V < 1 || V > TC_MAX_VOCAB || hist_len < 0 || hist_stride < hist_len)
        return fail(OPUS_ESHAPE, "debug_token_constraint: B=%d (max_batch %d) V=%d history %d (stride %d)", B, c->cfg.max_batch, V,
                    hist_len, hist_stride);
    if (c->cons_max_id >= V) return fail(OPUS_ESHAPE, "debug_token_constraint: the table holds id %d, V=%d", c->cons_max_id, V);
    if (c->cons_n_start != 1 && c->cons_n_start != B)
        return fail(OPUS_ESHAPE, "debug_token_constraint: %d per-row start states, %d rows", c->cons_n_start, B);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    OPC(set_cons_start_div(c, 1, s));
    for (int32_t t = 0; t < hist_len; ++t) {
        HIPC(launch_upload_i32(&t, 1, c->d_cstep, s));
        HIPC(launch_token_constraint(nullptr, B, V, d_hist, hist_stride, c->d_cstep, hist_len, c->d_cons, s));
    }
    HIPC(launch_upload_i32(&hist_len, 1, c->d_cstep, s));
    KL(KC_CONSTRAINT, 4.0 * B * V, launch_token_constraint(d_logits, B, V, d_hist, hist_stride, c->d_cstep, hist_len, c->d_cons, s));
    if (d_state_out)                         // (the state words are double-buffered by the step's parity)
        HIPC(hipMemcpyAsync(d_state_out, c->d_cstate + (hist_len & 1) * c->cfg.max_batch, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

extern "C" int opus_generate_greedy(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                                    int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id,
                                    int32_t *d_out_ids, int32_t *n_out, void *stream) {
    return generate_impl(c, d_embeds, d_mask, B, T, max_new, eos_ids, n_eos, pad_id, 0.f, 1.f, 0, d_out_ids, n_out, stream);
}

extern "C" int opus_generate_sample(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                                    int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature,
                                    float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out, void *stream) {
    if (!(temperature > 0.f)) return fail(OPUS_EBADARG, "generate_sample: temperature must be > 0 (use opus_generate_greedy)");
    return generate_impl(c, d_embeds, d_mask, B, T, max_new, eos_ids, n_eos, pad_id, temperature, top_p, seed, d_out_ids, n_out,
                         stream);
}

/* opus_generate_greedy (temperature == 0) / opus_generate_sample (temperature > 0) with per-step outputs, each optional (NULL =
   off): d_token_logprobs fp32 [B, max_new] (log-probability of the chosen token under the model's distribution; 0 after a row
   has finished), d_scores fp32 [max_new, B, V] (greedy: the logits; sampling: logits / T, -inf where the draw's top-k / top-p
   filters removed the token), d_logits fp32 [max_new, B, V] (the raw logits).  Steps past *n_out are not defined.  All NULL: the
   plain call, the same launches and graph. */
extern "C" int opus_generate_scored(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                                    const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature, float top_p,
                                    uint64_t seed, int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs, float *d_scores,
                                    float *d_logits, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!(temperature >= 0.f)) return fail(OPUS_EBADARG, "generate_scored: temperature must be >= 0 (0 = greedy)");
    const GenOutDesc outs{d_token_logprobs, d_scores, d_logits, nullptr};
    return generate_impl(c, d_embeds, d_mask, B, T, max_new, eos_ids, n_eos, pad_id, temperature, temperature > 0.f ? top_p : 1.f,
                         temperature > 0.f ? seed : 0, d_out_ids, n_out, stream, &outs);
}

/* opus_generate_scored on B prompts with nret decoder rows each: one prefill of the B prompts (opus_llama_prefill_fanout), then the
   loop of a B nret-row batch - decoder row r = b nret + j is the j-th sample of prompt b, its draws keyed by (seed, r, step).  The
   ids and the outputs are sized by B nret rows.  nret == 1: exactly opus_generate_scored. */
extern "C" int opus_generate_scored_fanout(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t nret,
                                           int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature,
                                           float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs,
                                           float *d_scores, float *d_logits, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!(temperature >= 0.f)) return fail(OPUS_EBADARG, "generate_scored_fanout: temperature must be >= 0 (0 = greedy)");
    const GenOutDesc outs{d_token_logprobs, d_scores, d_logits, nullptr};
    return generate_impl(c, d_embeds, d_mask, B, T, max_new, eos_ids, n_eos, pad_id, temperature, temperature > 0.f ? top_p : 1.f,
                         temperature > 0.f ? seed : 0, d_out_ids, n_out, stream, &outs, nret);
}

/* opus_generate_scored with classifier-free guidance on paired rows: d_embeds [2 P, T, D] / d_mask [2 P, T] hold the P conditional
   prompts, then their P negative prompts (left-padded to one length); one 2 P-row prefill, then the loop of a 2 P-row batch whose head
   works on the first P rows (select_next()).  ids and outputs are P-row shaped.  The scale travels in a device word: only "guided"
   enters the captured step's identity. */
extern "C" int opus_generate_scored_guided(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t P, int32_t T,
                                           float guidance_scale, int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id,
                                           float temperature, float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out,
                                           float *d_token_logprobs, float *d_scores, float *d_logits, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!(temperature >= 0.f)) return fail(OPUS_EBADARG, "generate_scored_guided: temperature must be >= 0 (0 = greedy)");
    if (!std::isfinite(guidance_scale)) return fail(OPUS_EBADARG, "generate_scored_guided: guidance_scale must be a finite number");
    if (P < 1 || 2 * (int64_t)P > c->cfg.max_batch)
        return fail(OPUS_ESHAPE, "generate_scored_guided: 2 x P = 2 x %d decoder rows, the context holds max_batch=%d", P, c->cfg.max_batch);
    const GenOutDesc outs{d_token_logprobs, d_scores, d_logits, nullptr};
    return generate_impl(c, d_embeds, d_mask, 2 * P, T, max_new, eos_ids, n_eos, pad_id, temperature, temperature > 0.f ? top_p : 1.f,
                         temperature > 0.f ? seed : 0, d_out_ids, n_out, stream, &outs, 1, nullptr, &guidance_scale);
}

/* Diagnostic: the guidance launches alone on caller memory - fp32 logits [2 P, V] (any P >= 1, any V >= 1, no alignment), rows
   [0, P) overwritten with the guided scores of the pairs (b, P + b), rows [P, 2 P) untouched.  Pairs are taken max_batch at a time:
   the log-sum-exp pass of the conditional rows, that of their partners, the combine. */
extern "C" int opus_debug_guidance(opus_ctx *c, float *d_logits, int32_t P, int32_t V, float guidance_scale, void *stream) {
    if (!c || !d_logits) return fail(OPUS_EBADARG, "debug_guidance: null pointer");
    if (P < 1 || V < 1) return fail(OPUS_ESHAPE, "debug_guidance: P=%d V=%d", P, V);
    if (!std::isfinite(guidance_scale)) return fail(OPUS_EBADARG, "debug_guidance: guidance_scale must be a finite number");
    HIPC(hipSetDevice(c->device));
    OPC(ensure_guid_mem(c, false));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    OPC(upload_guidance_scale(c, guidance_scale, s));
    const int Bm = c->cfg.max_batch;
    for (int b0 = 0; b0 < P; b0 += Bm) {
        const int n = P - b0 < Bm ? P - b0 : Bm;
        float *cond = d_logits + (size_t)b0 * V, *unc = d_logits + ((size_t)P + b0) * V;
        KL(KC_GUIDANCE, 4.0 * n * V, launch_guidance_lse_partial(cond, n, V, c->d_pval, c->d_gdpsum, s));
        KL(KC_GUIDANCE, 512.0 * n, launch_guidance_lse_final(c->d_pval, c->d_gdpsum, n, c->d_gmax, c->d_glog, c->d_glse, s));
        KL(KC_GUIDANCE, 4.0 * n * V, launch_guidance_lse_partial(unc, n, V, c->d_pval, c->d_gdpsum, s));
        KL(KC_GUIDANCE, 512.0 * n, launch_guidance_lse_final(c->d_pval, c->d_gdpsum, n, c->d_gmax + Bm, c->d_glog + Bm, c->d_glse + Bm, s));
        KL(KC_GUIDANCE, 12.0 * n * V,
           launch_guidance_combine(cond, unc, n, V, c->d_gmax, c->d_glog, c->d_gmax + Bm, c->d_glog + Bm, c->d_gscale, nullptr, s));
    }
    return OPUS_OK;
}

/* opus_generate_scored with its prefill replaced by opus_llama_prefill_behind: R suffix rows of n right-padded positions behind the
   rows h_src of a detached prefix.  Everything behind the prefill - the captured step and its cache key (R rows), EOS ids, stop
   sequence, processors, constraint, outputs, the draws keyed by (seed, row, step) - is that of an R-row batch. */
extern "C" int opus_generate_scored_behind(opus_ctx *c, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                           const int32_t *h_lens, const int32_t *h_src, int32_t max_new, const int32_t *eos_ids,
                                           int32_t n_eos, int32_t pad_id, float temperature, float top_p, uint64_t seed,
                                           int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs, float *d_scores, float *d_logits,
                                           void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!snap || !h_lens || !h_src || !d_embeds) return fail(OPUS_EBADARG, "generate_scored_behind: null pointer");
    if (!(temperature >= 0.f)) return fail(OPUS_EBADARG, "generate_scored_behind: temperature must be >= 0 (0 = greedy)");
    const GenOutDesc outs{d_token_logprobs, d_scores, d_logits, nullptr};
    const BehindArgs behind{snap, h_lens, h_src};
    return generate_impl(c, d_embeds, nullptr, R, n, max_new, eos_ids, n_eos, pad_id, temperature, temperature > 0.f ? top_p : 1.f,
                         temperature > 0.f ? seed : 0, d_out_ids, n_out, stream, &outs, 1, &behind);
}

// ------------------------------------------------------------------------------------------------ prompt-lookup decoding
// generate(prompt_lookup_num_tokens=k): per pass the rows' n-gram drafts (lookup_draft_kernel) are verified by ONE run of the
// layer loop on R n positions - prefill() with continuation rows behind the context's OWN cache (source rows the identity, Tp the
// host's mirror of T0 + step, every row appends its n positions) - then the final norm and lm_head on all R n rows, the arg-max and
// lookup_accept_kernel, which commits a + 1 ids per row in lockstep and advances the step word.  The host reads the pass's words
// back once (one synchronisation per pass, as beam search).  Slots beyond Tp + a keep the K / V of rejected positions: finite
// values no kernel reads, because attn_decode_kernel and attn_prefix_kernel select the visible slots by index (a slot past the
// end is never loaded in the first, is staged as zeros and set to -inf by a select in the second) and the next pass or step
// overwrites them before the end moves past them.
static int ensure_lookup_mem(opus_ctx *c) {
    if (c->lk_mem) return OPUS_OK;
    const size_t B = c->cfg.max_batch, row = align_up(B * sizeof(int32_t));
    HIPC(hipMalloc((void **)&c->lk_mem, 4 * row + align_up(80 * sizeof(int32_t)) + align_up(8 * sizeof(int32_t))));
    HIPC(hipMemset(c->lk_mem, 0, 4 * row + align_up(80 * sizeof(int32_t)) + align_up(8 * sizeof(int32_t))));
    c->d_lk_tok = reinterpret_cast<int32_t *>(c->lk_mem);
    c->d_lk_dlen = reinterpret_cast<int32_t *>(c->lk_mem + row);
    c->d_lk_hlen = reinterpret_cast<int32_t *>(c->lk_mem + 2 * row);
    c->d_lk_arg = reinterpret_cast<int32_t *>(c->lk_mem + 3 * row);
    c->d_lk_ids = reinterpret_cast<int32_t *>(c->lk_mem + 4 * row);
    c->d_lk_words = reinterpret_cast<int32_t *>(c->lk_mem + 4 * row + align_up(80 * sizeof(int32_t)));
    HIPC(hipHostMalloc((void **)&c->h_lk, 8 * sizeof(int32_t), hipHostMallocDefault));
    return OPUS_OK;
}

// host copy of the current prefill's kstart (the pass's rotary positions and attention tables are built on the host)
static int lookup_kstart(opus_ctx *c, hipStream_t s) {
    if (c->lk_epoch == c->epoch && (int)c->lk_kstart.size() == c->cur_B) return OPUS_OK;
    c->lk_kstart.assign((size_t)c->cur_B, 0);
    HIPC(hipMemcpyAsync(c->lk_kstart.data(), c->d_kstart, (size_t)c->cur_B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    c->lk_epoch = c->epoch;
    return OPUS_OK;
}

// One verify pass on the current decode state: tokens x [R, ld_x] (n columns used) at slots Tp .. Tp + n - 1 of every row; leaves
// the logits of all R n positions in d_logits (row r n + j) and the positions' K / V in the cache.  The step word is not touched.
static int verify_pass(opus_ctx *c, hipStream_t s, const int32_t *x, int ld_x, int n, int Tp) {
    const opus_config &g = c->cfg;
    const int R = c->cur_B, M = R * n, H = g.dec_dim, V = g.dec_vocab, G = g.dec_heads / g.dec_kv_heads;
    if (!c->behind_tbl) HIPC(hipMalloc((void **)&c->behind_tbl, (size_t)behind_table_words(g) * sizeof(int32_t)));
    std::vector<int32_t> src((size_t)R);
    for (int r = 0; r < R; ++r) src[r] = r;
    PrefixTables t;
    build_prefix_tables(g, c->lk_kstart, Tp, src.data(), R, n, t);
    if (t.nblocks > attn_prefix_max_blocks(R, g.max_batch, G, n)) return fail(OPUS_EHIP, "verify pass: block table overflow");
    const int o_lens = (int)t.w.size();
    t.w.insert(t.w.end(), (size_t)R, n);                                      // every row appends all its n positions
    if ((int64_t)t.w.size() > behind_table_words(g)) return fail(OPUS_EHIP, "verify pass: table overflow");
    int32_t *tbl = c->behind_tbl;
    c->phase = PH_DECODE;
    HIPC(launch_upload_i32(t.w.data(), (int)t.w.size(), tbl, s));
    // the input rows in the operand type, staged in d_xn (prefill() reads them into d_x before its first GEMM writes d_xn)
    KL(KC_OTHER, 4.0 * M * H, launch_lookup_embed(x, ld_x, R, n, c->dec_emb, H, V, c->d_xn, s));
    ContRows cr;
    cr.nkst = tbl + t.nkst;
    cr.nblocks = t.nblocks;
    cr.attn = prefix_params(c, tbl, t, Tp, n, c->d_qkv, nullptr, nullptr, c->d_ctx);
    cr.app_lens = tbl + o_lens;
    cr.w8 = true;
    OPC(prefill(c, s, c->d_xn, nullptr, R, n, true, &cr));
    c->phase = PH_DECODE;
    if (g.dec_arch == 1) {
        KL(KC_NORM, 6.0 * M * H, launch_layernorm(c->d_x, c->dec_lnfw, c->dec_lnfb, g.dec_rms_eps, M, H, c->d_xn, nullptr, s));
        OPC(gemm(c, s, c->d_xn, H, c->lm_head, M, V, H, nullptr, EPI_NONE, nullptr, c->d_logits, V, 1));
    } else {
        ResidShadow none;
        OPC(gemm_norm(c, s, none, c->d_x, g.dec_rms_eps, c->d_xn, c->lm_head, M, V, H, EPI_NONE, c->d_logits, V, 1));
    }
    ++c->lookup_passes;
    return OPUS_OK;
}

// arg-max of the first `rows` rows of d_logits -> out [rows]
static int lookup_argmax(opus_ctx *c, hipStream_t s, int rows, int32_t *out) {
    const int V = c->cfg.dec_vocab;
    KL(KC_OTHER, 4.0 * rows * V, launch_argmax_partial(c->d_logits, rows, V, c->d_pval, c->d_pidx, s));
    KL(KC_OTHER, 512.0 * rows, launch_lookup_argmax(c->d_pval, c->d_pidx, rows, out, s));
    return OPUS_OK;
}

// the pass's words -> pinned host memory, one synchronisation
static int lookup_words(opus_ctx *c, hipStream_t s, int nwords) {
    HIPC(hipMemcpyAsync(c->h_lk, c->d_lk_words, (size_t)nwords * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return OPUS_OK;
}

static int check_lookup_state(opus_ctx *c, const char *who) {
    if (!c->prefilled) return fail(OPUS_ESTATE, "%s before prefill", who);
    if (c->st.on) return fail(OPUS_ESTATE, "%s: a continuous session is open on this context", who);
    if (c->cur_B > 64) return fail(OPUS_ESHAPE, "%s: %d decoder rows (at most 64)", who, c->cur_B);
    return OPUS_OK;
}

extern "C" int opus_llama_verify_step(opus_ctx *c, const int32_t *d_tokens, int32_t n, const int32_t *d_draft_len, float *d_logits_all,
                                      int32_t *d_argmax, int32_t *a, void *stream) {
    OPC(need_ready(c));
    OPC(check_lookup_state(c, "verify_step"));
    if (!d_tokens || !a) return fail(OPUS_EBADARG, "verify_step: null pointer");
    const opus_config &g = c->cfg;
    const int R = c->cur_B;
    if (n < 1 || (int64_t)R * n > g.max_batch)
        return fail(OPUS_ESHAPE, "verify_step: R x n = %d x %d logits rows, the context holds max_batch=%d", R, n, g.max_batch);
    hipStream_t s = (hipStream_t)stream;
    OPC(ensure_lookup_mem(c));
    int32_t st = 0;
    HIPC(hipMemcpyAsync(&st, c->d_step, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (st < 0 || st + n > g.max_new_tokens)
        return fail(OPUS_ESHAPE, "verify_step: %d steps + %d positions, the KV cache holds max_new_tokens=%d behind the prompt", st, n,
                    g.max_new_tokens);
    OPC(lookup_kstart(c, s));
    OPC(verify_pass(c, s, d_tokens, n, n, c->cur_T + st));
    int32_t *arg = d_argmax ? d_argmax : c->d_lk_arg;
    OPC(lookup_argmax(c, s, R * n, arg));
    LookupAcceptParams p{};
    p.y = arg; p.x = d_tokens; p.ld_x = n; p.draft_len = d_draft_len; p.R = R; p.n = n; p.pre = 1;
    p.step = c->d_step; p.words = c->d_lk_words;
    KL(KC_OTHER, 8.0 * R * n, launch_lookup_accept(p, s));
    if (d_logits_all)
        HIPC(hipMemcpyAsync(d_logits_all, c->d_logits, (size_t)R * n * g.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    OPC(lookup_words(c, s, 4));
    *a = c->h_lk[0];
    return handoff_check(c, s);
}

extern "C" int opus_generate_lookup(opus_ctx *c, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                                    const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, int32_t k, int32_t max_ngram,
                                    const int32_t *d_hist, int32_t Lh, const int32_t *h_hist_len, int32_t *d_out_ids, int32_t *n_out,
                                    int64_t *stats, void *stream) {
    OPC(need_ready(c));
    OPC(check_prefill_args(c, d_embeds, d_mask, B, T));
    if (!d_out_ids || !n_out || !d_hist || !h_hist_len) return fail(OPUS_EBADARG, "generate_lookup: null pointer");
    const opus_config &g = c->cfg;
    if (k < 1 || B > 64 || (int64_t)B * (k + 1) > g.max_batch)
        return fail(OPUS_ESHAPE, "generate_lookup: a pass of B x (k + 1) = %d x %d logits rows needs max_batch >= %d (the context holds %d; "
                                 "at most 64 rows)", B, k + 1, B * (k + 1), g.max_batch);
    if (max_ngram < 1 || max_ngram > lookup_max_ngram())
        return fail(OPUS_EBADARG, "generate_lookup: max_matching_ngram_size=%d outside [1, %d]", max_ngram, lookup_max_ngram());
    if (Lh < 1) return fail(OPUS_EBADARG, "generate_lookup: history stride %d", Lh);
    for (int b = 0; b < B; ++b)
        if (h_hist_len[b] < 0 || h_hist_len[b] > Lh) return fail(OPUS_EBADARG, "generate_lookup: history length %d of row %d outside [0, %d]", h_hist_len[b], b, Lh);
    if (c->lproc_on || c->cons_on)
        return fail(OPUS_EUNSUPPORTED, "generate_lookup: logits processors / a token constraint are set on this context");
    hipStream_t s = (hipStream_t)stream;
    OPC(ensure_lookup_mem(c));
    const uint64_t seed = 0;
    OPC(begin_generation(c, "generate_lookup", 0.f, 1.f, max_new, eos_ids, n_eos, &seed, B, max_new, s));
    OPC(prefill(c, s, (const half_t *)d_embeds, d_mask, B, T));
    HIPC(launch_upload_i32(h_hist_len, B, c->d_lk_hlen, s));
    OPC(lookup_kstart(c, s));                                                 // (synchronises: the uploads above are done)
    int64_t passes = 0, plain = 0, drafted = 0, accepted = 0;
    LookupAcceptParams p{};
    p.y = c->d_lk_arg; p.x = c->d_lk_tok; p.ld_x = k + 1; p.draft_len = c->d_lk_dlen; p.R = B;
    p.ids = d_out_ids; p.stride = max_new; p.fin = c->d_fin; p.eos = c->d_eos; p.stop = c->d_stop; p.n_eos = n_eos; p.n_stop = c->n_stop;
    p.pad = pad_id; p.step = c->d_step; p.next = c->d_next; p.n_unf = c->d_nunf; p.words = c->d_lk_words; p.max_len = c->d_lk_words + 4;
    // behind every commit: the next pass's token matrix (the last committed id | the draft) and the longest draft, then the words
    auto commit = [&](int n, int pre) -> int {
        c->phase = PH_DECODE;
        OPC(lookup_argmax(c, s, B * n, c->d_lk_arg));
        p.n = n; p.pre = pre;
        KL(KC_OTHER, 8.0 * B * n, launch_lookup_accept(p, s));
        KL(KC_OTHER, 4.0 * B * (Lh + max_new), launch_lookup_draft(d_hist, Lh, c->d_lk_hlen, d_out_ids, max_new, c->d_step, 1, c->d_fin, B, k,
                                                                   max_ngram, pad_id, c->d_lk_tok + 1, k + 1, c->d_lk_tok, c->d_lk_dlen,
                                                                   c->d_lk_words + 4, s));
        return lookup_words(c, s, 5);
    };
    // x for a plain step's commit: column 0 of the token matrix is not compared (n = 1)
    OPC(commit(1, 0));                                                        // the first id, from the prefill's logits
    int S = 0;
    while (S + 1 < max_new && c->h_lk[1] > 0) {
        const int n = std::min(1 + c->h_lk[4], max_new - 1 - S);
        ++c->decode_steps;
        if (n <= 1) {                                                         // no unfinished row has a draft: one plain decode step
            OPC(decode_step(c, s, c->d_next));
            OPC(commit(1, 0));
            ++plain;
        } else {
            OPC(verify_pass(c, s, c->d_lk_tok, k + 1, n, T + S));
            OPC(commit(n, 1));
            ++passes;
            drafted += c->h_lk[3];
            accepted += c->h_lk[0];
        }
        S = c->h_lk[2];
    }
    const int produced = S + 1;
    std::vector<int32_t> nunf((size_t)produced, 1);
    HIPC(hipMemcpyAsync(nunf.data(), c->d_nunf, (size_t)produced * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OPC(handoff_check(c, s));                                                 // (synchronises the stream)
    int nn = produced;
    for (int q = 0; q < produced; ++q) if (nunf[q] == 0) { nn = q + 1; break; }
    *n_out = nn;
    if (stats) { stats[0] = passes; stats[1] = plain; stats[2] = drafted; stats[3] = accepted; }
    return OPUS_OK;
}

extern "C" int opus_debug_lookup_draft(opus_ctx *c, const int32_t *d_hist, int32_t Lh, const int32_t *d_hist_len, int32_t R, int32_t k,
                                       int32_t max_ngram, int32_t *d_draft, int32_t *d_draft_len, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!d_hist || !d_hist_len || !d_draft || !d_draft_len) return fail(OPUS_EBADARG, "debug_lookup_draft: null pointer");
    if (R < 1 || k < 1 || Lh < 1 || max_ngram < 1 || max_ngram > lookup_max_ngram())
        return fail(OPUS_EBADARG, "debug_lookup_draft: R=%d k=%d Lh=%d max_ngram=%d (at most %d)", R, k, Lh, max_ngram, lookup_max_ngram());
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    KL(KC_OTHER, 4.0 * R * Lh, launch_lookup_draft(d_hist, Lh, d_hist_len, nullptr, 0, nullptr, 0, nullptr, R, k, max_ngram, 0, d_draft, k,
                                                    nullptr, d_draft_len, nullptr, s));
    return OPUS_OK;
}

extern "C" int opus_debug_last_qkv(opus_ctx *c, void *d_out, int32_t rows, void *stream) {
    if (!c || !d_out) return fail(OPUS_EBADARG, "debug_last_qkv: null pointer");
    const opus_config &g = c->cfg;
    if (rows < 1 || rows > dec_rows_cap(g)) return fail(OPUS_ESHAPE, "debug_last_qkv: rows=%d (1 .. %lld)", rows, (long long)dec_rows_cap(g));
    HIPC(hipSetDevice(c->device));
    const size_t QKV = (size_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim;
    HIPC(hipMemcpyAsync(d_out, c->d_qkv, (size_t)rows * QKV * sizeof(half_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return OPUS_OK;
}

extern "C" int opus_debug_lookup_accept(opus_ctx *c, const int32_t *d_argmax, const int32_t *d_tokens, const int32_t *d_draft_len, int32_t R,
                                        int32_t n, int32_t pre, int32_t *d_ids, int32_t stride, int32_t *d_fin, int32_t *d_step,
                                        const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, const int32_t *stop_ids, int32_t n_stop,
                                        int32_t *d_next, int32_t *d_nunf, int32_t *h_words, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (!d_argmax || !d_tokens || !d_ids || !d_fin || !d_step || !d_next || !d_nunf || !h_words)
        return fail(OPUS_EBADARG, "debug_lookup_accept: null pointer");
    if (R < 1 || R > 64 || n < 1 || stride < 1 || n_eos < 0 || n_eos > 64 || n_stop < 0 || n_stop > 8 || (pre != 0 && pre != 1) ||
        (pre == 0 && n != 1) || (n_eos && !eos_ids) || (n_stop && !stop_ids))
        return fail(OPUS_EBADARG, "debug_lookup_accept: R=%d n=%d stride=%d n_eos=%d n_stop=%d pre=%d", R, n, stride, n_eos, n_stop, pre);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    OPC(ensure_lookup_mem(c));
    if (n_eos) HIPC(launch_upload_i32(eos_ids, n_eos, c->d_lk_ids, s));
    if (n_stop) HIPC(launch_upload_i32(stop_ids, n_stop, c->d_lk_ids + 64, s));
    LookupAcceptParams p{};
    p.y = d_argmax; p.x = d_tokens; p.ld_x = n; p.draft_len = d_draft_len; p.R = R; p.n = n; p.pre = pre; p.ids = d_ids; p.stride = stride;
    p.fin = d_fin; p.eos = c->d_lk_ids; p.stop = c->d_lk_ids + 64; p.n_eos = n_eos; p.n_stop = n_stop; p.pad = pad_id; p.step = d_step;
    p.next = d_next; p.n_unf = d_nunf; p.words = c->d_lk_words;
    KL(KC_OTHER, 8.0 * R * n, launch_lookup_accept(p, s));
    OPC(lookup_words(c, s, 4));
    for (int i = 0; i < 4; ++i) h_words[i] = c->h_lk[i];
    return OPUS_OK;
}

/* Diagnostic: the fused arg-max / log-sum-exp pass of opus_generate_scored on fp32 logits [B, V] (B <= max_batch, any V >= 1):
   d_idx [B] (the arg-max argmax_partial gives: lowest index among ties), d_lse [B]. */
extern "C" int opus_debug_argmax_lse(opus_ctx *c, const float *d_logits, int32_t B, int32_t V, int32_t *d_idx, float *d_lse,
                                     void *stream) {
    if (!c || !d_logits || !d_idx || !d_lse) return fail(OPUS_EBADARG, "debug_argmax_lse: null pointer");
    if (B < 1 || B > c->cfg.max_batch || V < 1) return fail(OPUS_ESHAPE, "debug_argmax_lse: B=%d (max_batch %d) V=%d", B, c->cfg.max_batch, V);
    HIPC(hipSetDevice(c->device));
    OPC(ensure_gen_mem(c));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    KL(KC_OTHER, 4.0 * B * V, launch_argmax_lse_partial(d_logits, B, V, c->d_pval, c->d_pidx, c->d_gpsum, s));
    KL(KC_OTHER, 512.0 * B, launch_argmax_lse_final(c->d_pval, c->d_pidx, c->d_gpsum, B, d_idx, d_lse, s));
    return OPUS_OK;
}

/* The k likeliest tokens of every step's raw row (topk.hip) for the opus_generate_scored* calls of this context, and of every scored
   row for opus_llama_forward, until cleared with k = 0.  generate: d_top_ids int32 / d_top_lp fp32 [rows, max_new, k], rows those of
   the call's other outputs; a row that had finished before a step gets ids -1 and log-probs 0.  forward: [R, k] in the order of
   d_rows.  The raw row is the one d_token_logprobs describes (before guidance, processors, constraint, temperature, warpers; the
   conditional row under guidance).  Only "on" enters the captured step's identity: k and the addresses travel in the descriptor. */
extern "C" int opus_set_gen_top_logprobs(opus_ctx *c, int32_t k, int32_t *d_top_ids, float *d_top_lp) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (k < 0 || k > TOPK_MAX || k > c->cfg.dec_vocab)
        return fail(OPUS_EBADARG, "set_gen_top_logprobs: k=%d outside 0..%d (dec_vocab %d)", k, TOPK_MAX, c->cfg.dec_vocab);
    if (k > 0 && (!d_top_ids || !d_top_lp)) return fail(OPUS_EBADARG, "set_gen_top_logprobs: null buffer");
    c->top_k = k;
    c->top_ids = k ? d_top_ids : nullptr;
    c->top_lp = k ? d_top_lp : nullptr;
    return OPUS_OK;
}

/* Diagnostic: the two top-k stages alone on caller rows - d_logits [R, ld] of dtype OPUS_F32 or OPUS_F16 (the build's 16-bit type),
   V <= ld values a row, any R >= 1, 1 <= k <= min(20, V); d_ids int32 / d_lp fp32 [R, k].  d_lse [R] or NULL: the rows'
   log-sum-exp is computed here (contiguous fp32 rows: the fused arg-max / log-sum-exp pass of the decode step). */
extern "C" int opus_debug_top_logprobs(opus_ctx *c, const void *d_logits, int32_t dtype, int64_t ld, int32_t R, int32_t V, int32_t k,
                                       const float *d_lse, int32_t *d_ids, float *d_lp, void *stream) {
    if (!c || !d_logits || !d_ids || !d_lp) return fail(OPUS_EBADARG, "debug_top_logprobs: null pointer");
    if (dtype != OPUS_F32 && dtype != OPUS_F16) return fail(OPUS_EBADARG, "debug_top_logprobs: dtype %d (OPUS_F32 or OPUS_F16)", dtype);
    if (R < 1 || V < 1 || ld < V) return fail(OPUS_ESHAPE, "debug_top_logprobs: R=%d V=%d ld=%lld", R, V, (long long)ld);
    if (k < 1 || k > TOPK_MAX || k > V) return fail(OPUS_EBADARG, "debug_top_logprobs: k=%d outside 1..min(%d, V=%d)", k, TOPK_MAX, V);
    HIPC(hipSetDevice(c->device));
    OPC(ensure_gen_mem(c));
    OPC(ensure_topk_mem(c));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    const bool f32 = dtype == OPUS_F32;
    const int Bm = c->cfg.max_batch;                                   // (d_pval / d_gpsum hold max_batch rows)
    for (int r0 = 0; r0 < R; r0 += Bm) {
        const int n = R - r0 < Bm ? R - r0 : Bm;
        const char *rows = (const char *)d_logits + (size_t)r0 * ld * (f32 ? sizeof(float) : sizeof(half_t));
        TopkArgs ta;
        ta.cand = c->d_tcand; ta.k = k; ta.ids = d_ids + (size_t)r0 * k; ta.lp = d_lp + (size_t)r0 * k;
        if (d_lse) {
            ta.lse = d_lse + r0;
        } else if (f32 && ld == V) {
            KL(KC_OTHER, 4.0 * n * V, launch_argmax_lse_partial((const float *)rows, n, V, c->d_pval, c->d_pidx, c->d_gpsum, s));
            ta.pval = c->d_pval; ta.psum = c->d_gpsum;
        } else {
            KL(KC_OTHER, (f32 ? 8.0 : 4.0) * n * V, launch_topk_row_lse(rows, f32, ld, n, V, c->d_tlse, s));
            ta.lse = c->d_tlse;
        }
        if (f32) KL(KC_TOPK, 4.0 * n * V, launch_topk_f32((const float *)rows, ld, n, V, ta, s));
        else KL(KC_TOPK, 2.0 * n * V, launch_topk_h16((const half_t *)rows, ld, n, V, ta, s));
    }
    return OPUS_OK;
}

/* Diagnostic: one draw per row from fp32 logits [B,V] with the sampling head (step counter = `step`). */
extern "C" int opus_debug_sample(opus_ctx *c, const float *d_logits, int32_t B, float temperature, float top_p, uint64_t seed,
                                 int32_t step, int32_t *d_tokens, void *stream) {
    if (!c || !d_logits || !d_tokens) return fail(OPUS_EBADARG, "debug_sample: null pointer");
    if (B < 1 || B > c->cfg.max_batch || !(temperature > 0.f) || top_p <= 0.f || top_p > 1.f) return fail(OPUS_EBADARG, "debug_sample: argument");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemcpyAsync(c->d_seed, &seed, sizeof(seed), hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c->d_plan, &step, sizeof(step), hipMemcpyHostToDevice, s));
    if (c->warp_on()) {
        OPC(upload_warpers(c, s));
        HIPC(launch_sample_select(d_logits, B, c->cfg.dec_vocab, temperature, top_p, c->samp_top_k, nullptr, nullptr, c->d_pval, c->d_pidx,
                                  c->d_probs, c->d_cand_i, c->d_cand_n, c->d_zpart, c->d_spart, nullptr, c->d_wlo, nullptr, nullptr, s));
        HIPC(launch_sample_warp_draw(B, c->cfg.dec_vocab, c->d_warp, c->d_seed, c->d_plan, c->d_probs, c->d_cand_i, c->d_cand_n, d_tokens,
                                     c->d_wlo, c->d_whi, s));
    } else {
        HIPC(launch_sample_select(d_logits, B, c->cfg.dec_vocab, temperature, top_p, c->samp_top_k, c->d_seed, c->d_plan, c->d_pval, c->d_pidx,
                                  c->d_probs, c->d_cand_i, c->d_cand_n, c->d_zpart, c->d_spart, d_tokens, nullptr, nullptr, nullptr, s));
    }
    HIPC(hipStreamSynchronize(s));   // seed / step are host temporaries
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ diagnostics
extern "C" int opus_debug_gemm(opus_ctx *c, const void *A, const void *W, const float *bias, const float *residual,
                               void *Cp, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t out_f32, void *stream) {
    if (!c || !A || !W || !Cp) return fail(OPUS_EBADARG, "debug_gemm: null pointer");
    if (M < 1 || N < 1 || K < 64 || K % 64) return fail(OPUS_ESHAPE, "debug_gemm: K must be a positive multiple of 64");
    if (epi < 0 || epi > 2 || (epi == 2 && N % 32)) return fail(OPUS_EBADARG, "debug_gemm: epilogue");
    HIPC(hipSetDevice(c->device));
    const int nout = epi == EPI_SILU_GU16 ? N / 2 : N;
    // (tests: A handed over in fragment order, ceil(M / 16) * 16 rows)
    return gemm(c, (hipStream_t)stream, (const half_t *)A, K, (const half_t *)W, M, N, K, bias, epi, residual, Cp, nout,
                out_f32, GemmAsk().tiled_a(g_knobs.debug_a_tiled));
}

extern "C" int opus_debug_gemm_norm(opus_ctx *c, const float *A, const void *W, void *Cp, int32_t M, int32_t N, int32_t K,
                                    int32_t epi, int32_t out_f32, float eps, void *stream) {
    if (!c || !A || !W || !Cp) return fail(OPUS_EBADARG, "debug_gemm_norm: null pointer");
    if (M < 1 || M > MID_MAX_M || N < 1 || K < 64 || K % 64) return fail(OPUS_ESHAPE, "debug_gemm_norm: M <= 64, K %% 64 == 0");
    if (epi != 0 && epi != 2) return fail(OPUS_EBADARG, "debug_gemm_norm: epilogue 0 or 2");
    HIPC(hipSetDevice(c->device));
    const int nout = epi == EPI_SILU_GU16 ? N / 2 : N;
    return gemm_any(c, (hipStream_t)stream, nullptr, A, eps, K, (const half_t *)W, M, N, K, nullptr, epi, nullptr, Cp, nout,
                    out_f32);
}

// The ESM QKV projection + rotary exactly as opus_esm2_encode issues it: out[M, 3 D] fp16 = rotary(A W^T + bias) with the
// query third scaled by head_dim^-0.5, positions row % T.  allow_fuse = 0 forces the stand-alone rotary kernel on the stored
// projection; *fused (HOST) = 1 when the GEMM's epilogue did the rotation.
extern "C" int opus_debug_gemm_rope(opus_ctx *c, const void *A, const void *W, const float *bias, void *out, int32_t M,
                                    int32_t D, int32_t K, int32_t T, int32_t heads, int32_t allow_fuse, int32_t *fused,
                                    void *stream) {
    if (!c || !A || !W || !out || !fused) return fail(OPUS_EBADARG, "debug_gemm_rope: null pointer");
    if (M < 1 || D < 16 || K < 64 || K % 64 || T < 1 || heads < 1 || D % heads || M % T)
        return fail(OPUS_ESHAPE, "debug_gemm_rope: M %% T == 0, D %% heads == 0, K %% 64 == 0");
    const int hd = D / heads;
    if (hd != c->cfg.enc_dim / c->cfg.enc_heads || T > c->cfg.max_enc_tokens)
        return fail(OPUS_ESHAPE, "debug_gemm_rope: head_dim / T must match the context's encoder rotary table");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const float qs = 1.0f / sqrtf((float)hd);
    GemmGot got;
    OPC(gemm(c, s, (const half_t *)A, K, (const half_t *)W, M, 3 * D, K, bias, EPI_NONE, nullptr, out, 3 * D, 0,
             GemmAsk().rope(allow_fuse && hd == 64 ? c->cs_enc : nullptr, nullptr, T, D, qs), &got));
    *fused = got.rope_done;
    if (!got.rope_done) HIPC(launch_esm_rope((half_t *)out, c->cs_enc, M / T, T, heads, hd, qs, s));
    return OPUS_OK;
}

// The producer / consumer pair of the row-scale RMSNorm fusion exactly as prefill() and decode_step() issue it:
//   X <- X + A W1^T            (wo: a split-K GEMM whose reduce also writes fp16(X) and per-256-column sums of squares)
//   C  = epi(rmsnorm(X) W2^T)  (gate/up or lm_head: gemm_wide_kernel scales its rows by the rstd from those sums)
// *fused = 1 when the fused form ran (0: the separate-norm fallback ran; the result is the same function either way).
extern "C" int opus_debug_gemm_rowscale(opus_ctx *c, const void *A, const void *W1, float *X, const void *W2, void *Cp, int32_t M,
                                        int32_t N1, int32_t K1, int32_t N2, int32_t epi, float eps, int32_t *fused, void *stream) {
    if (!c || !A || !W1 || !X || !W2 || !Cp || !fused) return fail(OPUS_EBADARG, "debug_gemm_rowscale: null pointer");
    if (M < 1 || N1 < 64 || N1 % 64 || K1 < 64 || K1 % 64 || N2 < 32) return fail(OPUS_ESHAPE, "debug_gemm_rowscale: shape");
    if (epi != EPI_NONE && epi != EPI_SILU_GU16) return fail(OPUS_EBADARG, "debug_gemm_rowscale: epilogue 0 or 2");
    const opus_config &g = c->cfg;
    if ((int64_t)M * N1 > (int64_t)g.max_batch * g.max_prompt * g.dec_dim) return fail(OPUS_ESHAPE, "debug_gemm_rowscale: M * N1 exceeds the scratch");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    ResidShadow sh;
    GemmGot got;
    OPC(gemm(c, s, (const half_t *)A, K1, (const half_t *)W1, M, N1, K1, nullptr, EPI_NONE, X, X, N1, 1,
             GemmAsk().copy16(fuse_rows() && M <= 96 ? c->d_xn : nullptr), &got));
    sh.produced(X, got);
    *fused = sh.xh_src != nullptr && (N1 & 255) == 0 && gemm_goes_wide(M, N2) ? 1 : 0;
    const int nout = epi == EPI_SILU_GU16 ? N2 / 2 : N2;
    return gemm_norm(c, s, sh, X, eps, c->d_xn, (const half_t *)W2, M, N2, N1, epi, Cp, nout, 0);
}

// The norm fused around gemm_pp_kernel exactly as encode() (LayerNorm) and prefill() (RMSNorm) issue it:
//   X <- X + A W1^T (+ b1)       (fp32 in place; the epilogue / pair combine / tail reduce also writes fp16(X) and the partials)
//   stat = ln_finalize(part)     ((mu, rstd) per row; rms: (0, rsqrt(mean x^2 + eps)))
//   C  = epi(rstd (fp16(X) W2^T - mu s) + c2), optionally rotated (rope_T > 0: the ESM QKV form, N2 = 3 D)
// part / xh / stat are the caller's; plan (HOST) receives launch_pp's report of both GEMMs.  *produced = 0: the producer GEMM did
// not leave the partials (shape off gemm_pp_kernel's fused form) and nothing after it ran - no stand-alone fallback here.
extern "C" int opus_debug_gemm_ln(opus_ctx *c, const void *A, const void *W1, const float *b1, float *X, float *part, void *xh,
                                  float *stat, const void *W2, const float *c2, const float *colsum, void *Cp, int32_t M, int32_t N1,
                                  int32_t K1, int32_t N2, int32_t epi, int32_t rms, float eps, int32_t rope_T,
                                  const int32_t *rope_pos, int32_t *produced, int32_t *plan, void *stream) {
    if (!c || !A || !W1 || !X || !part || !xh || !stat || !W2 || !Cp || !produced || !plan)
        return fail(OPUS_EBADARG, "debug_gemm_ln: null pointer");
    if (M < 1 || N1 < 64 || N1 % 64 || K1 < 64 || K1 % 64 || N2 < 32) return fail(OPUS_ESHAPE, "debug_gemm_ln: shape");
    if (epi != EPI_NONE && epi != EPI_GELU && epi != EPI_SILU_GU16) return fail(OPUS_EBADARG, "debug_gemm_ln: epilogue 0, 1 or 2");
    if (epi == EPI_SILU_GU16 && (!rms || c2 || colsum || N2 % 32))
        return fail(OPUS_EBADARG, "debug_gemm_ln: the gate / up epilogue is the RMSNorm form (no bias, no column sums)");
    if (rms ? colsum != nullptr : colsum == nullptr) return fail(OPUS_EBADARG, "debug_gemm_ln: column sums go with LayerNorm only");
    if (rope_pos && rope_T < 1) return fail(OPUS_EBADARG, "debug_gemm_ln: rope_pos needs rope_T");
    if (rope_T > 0 && (epi != EPI_NONE || N2 % 3 || (N2 / 3) % 64 || c->cfg.enc_dim / c->cfg.enc_heads != 64 ||
                       rope_T > c->cfg.max_enc_tokens))
        return fail(OPUS_ESHAPE, "debug_gemm_ln: rotary needs EPI_NONE, N2 = 3 D, head_dim 64 and rope_T within the context's table");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_OTHER;
    for (int i = 0; i < 2 * PP_PLAN_WORDS; ++i) plan[i] = -1;
    HIPC(hipMemsetAsync(c->d_cnt, 0, HANDOFF_ERR * sizeof(int32_t), s));       // hand-off words start from zero, as at the head of encode / prefill
    GemmGot got;
    // (the partials are asked of the big tiled GEMM only, as the path does)
    OPC(gemm(c, s, (const half_t *)A, K1, (const half_t *)W1, M, N1, K1, b1, EPI_NONE, X, X, N1, 1,
             GemmAsk().ln_produce(gemm_goes_pp(M, N1) ? part : nullptr, (half_t *)xh).report_pp(plan), &got));
    *produced = got.ln_done;
    if (!got.ln_done) return OPUS_OK;
    KL(KC_NORM, 8.0 * M * (N1 / 64), launch_ln_finalize(part, M, N1 / 64, N1, eps, rms, stat, s));
    const int nout = epi == EPI_SILU_GU16 ? N2 / 2 : N2;
    OPC(gemm(c, s, (const half_t *)xh, N1, (const half_t *)W2, M, N2, N1, c2, epi, nullptr, Cp, nout, 0,
             GemmAsk().ln_consume(stat, colsum).report_pp(plan + PP_PLAN_WORDS)
                 .rope(rope_T > 0 ? c->cs_enc : nullptr, rope_pos, rope_T, N2 / 3, 0.125f), &got));   // (head_dim 64)
    if (rope_T > 0 && !got.rope_done) return fail(OPUS_ESTATE, "debug_gemm_ln: the consumer GEMM did not fuse the rotary");
    return OPUS_OK;
}

// The QKV projection of the batched decode step exactly as decode_step() issues it (narrow output routed through the
// k-part kernels, raw slabs left for the attention kernel): d_slabs fp32 [*ks][M][N] receives the slabs, *ks (HOST) their
// number; *ks = 1 means the launch wrote a finished fp16 output instead (nothing is copied).
extern "C" int opus_debug_gemm_slabs(opus_ctx *c, const void *A, const void *W, float *d_slabs, int32_t M, int32_t N, int32_t K,
                                     int32_t *ks, void *stream) {
    if (!c || !A || !W || !ks) return fail(OPUS_EBADARG, "debug_gemm_slabs: null pointer");   // (d_slabs may be NULL: timing runs)
    if (M < 1 || N < 16 || K < 64 || K % 64) return fail(OPUS_ESHAPE, "debug_gemm_slabs: shape");
    const opus_config &g = c->cfg;
    const int64_t QKVd = (int64_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim;
    if ((int64_t)M * N > (int64_t)g.max_batch * g.max_prompt * QKVd) return fail(OPUS_ESHAPE, "debug_gemm_slabs: M * N exceeds the scratch");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    GemmGot got;
    OPC(gemm(c, s, (const half_t *)A, K, (const half_t *)W, M, N, K, nullptr, EPI_NONE, nullptr, c->d_qkv, N, 0,
             GemmAsk().slabs().tiled_a(g_knobs.debug_a_tiled), &got));
    *ks = got.ks;
    if (got.ks > 1 && d_slabs)
        HIPC(hipMemcpyAsync(d_slabs, c->gemm_ws, (size_t)got.ks * M * N * sizeof(float), hipMemcpyDeviceToDevice, s));
    return OPUS_OK;
}

// opus_debug_gemm (form 0: A in the operand type), opus_debug_gemm_norm (form 1: A fp32, eps) or opus_debug_gemm_slabs (form 2:
// d_C = the slab buffer, *ks) with the quantised form `q` of W offered beside it, as decode_step() offers it: *ran (HOST) = 1 when
// the routed kernel streamed the quantised panels, 0 when it has no such form and read W.  `who`: the entry point, for the messages.
static int debug_gemm_wq(const char *who, opus_ctx *c, int32_t form, const void *A, const void *W, const QuantW &q,
                         const float *bias, const float *residual, void *Cp, int32_t M, int32_t N, int32_t K, int32_t epi,
                         int32_t out_f32, float eps, int32_t *ks, int32_t *ran, void *stream) {
    if (!c || !A || !W || !q.codes || !q.scales || !ran || (form != 2 && !Cp)) return fail(OPUS_EBADARG, "%s: null pointer", who);
    if (form < 0 || form > 2) return fail(OPUS_EBADARG, "%s: form 0, 1 or 2", who);
    if (M < 1 || N < 1 || K < 64 || K % 64) return fail(OPUS_ESHAPE, "%s: K must be a positive multiple of 64", who);
    if (epi < 0 || epi > 2 || (epi == 2 && N % 32)) return fail(OPUS_EBADARG, "%s: epilogue", who);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nout = epi == EPI_SILU_GU16 ? N / 2 : N;
    const GemmAsk ask = GemmAsk().quant(q);
    *ran = 0;
    if (form == 0) {
        OPC(gemm(c, s, (const half_t *)A, K, (const half_t *)W, M, N, K, bias, epi, residual, Cp, nout, out_f32,
                 GemmAsk(ask).tiled_a(g_knobs.debug_a_tiled)));
    } else if (form == 1) {
        if (M > MID_MAX_M) return fail(OPUS_ESHAPE, "%s: the fused norm takes M <= 64", who);
        if (epi == 1 || bias || residual) return fail(OPUS_EBADARG, "%s: the fused norm takes epilogue 0 or 2, no bias, no residual", who);
        OPC(gemm_any(c, s, nullptr, (const float *)A, eps, K, (const half_t *)W, M, N, K, nullptr, epi, nullptr, Cp, nout, out_f32, ask));
    } else {
        if (!ks || epi != 0 || N < 16) return fail(OPUS_EBADARG, "%s: the slab form takes ks, the plain epilogue and N >= 16", who);
        const opus_config &g = c->cfg;
        const int64_t QKVd = (int64_t)(g.dec_heads + 2 * g.dec_kv_heads) * g.dec_head_dim;
        if ((int64_t)M * N > (int64_t)g.max_batch * g.max_prompt * QKVd) return fail(OPUS_ESHAPE, "%s: M * N exceeds the scratch", who);
        GemmGot got;
        OPC(gemm(c, s, (const half_t *)A, K, (const half_t *)W, M, N, K, nullptr, EPI_NONE, nullptr, c->d_qkv, N, 0,
                 GemmAsk(ask).slabs().tiled_a(g_knobs.debug_a_tiled), &got));
        *ks = got.ks;
        if (got.ks > 1 && Cp)
            HIPC(hipMemcpyAsync(Cp, c->gemm_ws, (size_t)got.ks * M * N * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    *ran = c->gemm_wq == q.fmt;
    return OPUS_OK;
}
// The FP8 form of W (opus_quantize_fp8: d_q8, d_e8)
extern "C" int opus_debug_gemm_w8(opus_ctx *c, int32_t form, const void *A, const void *W, const void *q8, const void *e8,
                                  const float *bias, const float *residual, void *Cp, int32_t M, int32_t N, int32_t K, int32_t epi,
                                  int32_t out_f32, float eps, int32_t *ks, int32_t *ran, void *stream) {
    if ((((uintptr_t)q8) & 15) || (((uintptr_t)e8) & 3)) return fail(OPUS_EBADARG, "debug_gemm_w8: d_q8 must be 16-byte, d_e8 4-byte aligned");
    return debug_gemm_wq("debug_gemm_w8", c, form, A, W, QuantW{WQ_FP8, (const uint8_t *)q8, e8}, bias, residual, Cp, M, N, K,
                         epi, out_f32, eps, ks, ran, stream);
}
// The MXFP4 form of W (opus_quantize_mxfp4: d_q4, d_s4)
extern "C" int opus_debug_gemm_w4(opus_ctx *c, int32_t form, const void *A, const void *W, const void *q4, const void *s4,
                                  const float *bias, const float *residual, void *Cp, int32_t M, int32_t N, int32_t K, int32_t epi,
                                  int32_t out_f32, float eps, int32_t *ks, int32_t *ran, void *stream) {
    if ((((uintptr_t)q4) & 15) || (((uintptr_t)s4) & 15)) return fail(OPUS_EBADARG, "debug_gemm_w4: d_q4 and d_s4 must be 16-byte aligned");
    return debug_gemm_wq("debug_gemm_w4", c, form, A, W, QuantW{WQ_MXFP4, (const uint8_t *)q4, s4}, bias, residual, Cp, M, N, K,
                         epi, out_f32, eps, ks, ran, stream);
}

// What the launchers launched for the last GEMM issued on this context (opus_debug_gemm, opus_debug_gemm_norm,
// opus_debug_gemm_slabs or any path call): GemmParams::plan, GEMM_PLAN_WORDS ints to HOST memory; all -1: no GEMM yet, or the
// launcher refused the last one before it chose a kernel.
extern "C" int opus_debug_gemm_plan(opus_ctx *c, int32_t *plan) {
    if (!c || !plan) return fail(OPUS_EBADARG, "debug_gemm_plan: null pointer");
    for (int i = 0; i < GEMM_PLAN_WORDS; ++i) plan[i] = c->gemm_plan[i];
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ beam search support
// The best M continuations of every batch row over its K beams' last logits (this context's most recent prefill / decode step
// on B K rows, row = b K + k): transformers generation/utils.py _beam_search step b-c - log_softmax in fp32, + running beam
// scores, torch.topk over the flattened [K V] - scores fp32 [B, M] descending and flat indices k V + token int32 [B, M].
extern "C" int opus_beam_topk(opus_ctx *c, const float *d_run_scores, int32_t B, int32_t K, int32_t M, float *d_scores,
                              int32_t *d_idx, void *stream) {
    if (!c || !d_run_scores || !d_scores || !d_idx) return fail(OPUS_EBADARG, "beam_topk: null pointer");
    if (!c->prefilled) return fail(OPUS_ESTATE, "beam_topk before prefill");
    if (B < 1 || K < 1 || B * K != c->cur_B) return fail(OPUS_ESHAPE, "beam_topk: B=%d x K=%d rows, the last step had %d", B, K, c->cur_B);
    if (M < 1 || M > 16) return fail(OPUS_ESHAPE, "beam_topk: 1 <= M <= 16 candidates per row (got %d)", M);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->phase = PH_DECODE;
    KL(KC_OTHER, 12.0 * c->cur_B * c->cfg.dec_vocab,
       launch_beam_topk(c->d_logits, d_run_scores, B, K, c->cfg.dec_vocab, M, c->d_zpart, d_scores, d_idx, s));
    return OPUS_OK;
}

// Beam-sample step (do_sample with num_beams > 1; transformers _get_top_k_continuations, do_sample branch): the M
// continuations of every batch row drawn WITHOUT replacement from softmax over the K V accumulated log-probabilities, after
// log_softmax and the warpers (temperature, top_k of opus_set_sampling_top_k, top_p) on each of the K rows - scores fp32
// [B, M] (the accumulated log-probabilities of the drawn continuations) and flat indices k V + token int32 [B, M] in the order
// drawn; entries beyond the continuations of non-zero probability are -inf / 0x7fffffff.  d_logits NULL: the last step's.
extern "C" int opus_beam_sample_topk(opus_ctx *c, const float *d_logits, const float *d_run_scores, int32_t B, int32_t K, int32_t M,
                                     float temperature, float top_p, uint64_t seed, int32_t step, float *d_scores, int32_t *d_idx,
                                     void *stream) {
    if (!c || !d_run_scores || !d_scores || !d_idx) return fail(OPUS_EBADARG, "beam_sample_topk: null pointer");
    if (!d_logits && !c->prefilled) return fail(OPUS_ESTATE, "beam_sample_topk before prefill");
    if (B < 1 || K < 1 || B * K > c->cfg.max_batch || (!d_logits && B * K != c->cur_B))
        return fail(OPUS_ESHAPE, "beam_sample_topk: B=%d x K=%d rows (the last step had %d, the context holds %d)", B, K, c->cur_B, c->cfg.max_batch);
    if (M < 1 || M > 16) return fail(OPUS_ESHAPE, "beam_sample_topk: 1 <= M <= 16 candidates per row (got %d)", M);
    if (!(temperature > 0.f) || top_p <= 0.f || top_p > 1.f) return fail(OPUS_EBADARG, "beam_sample_topk: temperature > 0, 0 < top_p <= 1");
    if (c->warp_on())
        return fail(OPUS_EUNSUPPORTED, "beam_sample_topk: sampling warpers (opus_set_sampling_warpers) are set on this context; beam-sample "
                                       "needs min_tokens_to_keep = #eos + 1, i.e. M / K, and joint draws");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const float *lg = d_logits ? d_logits : c->d_logits;
    const int V = c->cfg.dec_vocab, R = B * K;
    c->phase = PH_DECODE;
    // min_tokens_to_keep of both warpers under beam-sample: #eos + 1, at least 2 (generation/utils.py _get_logits_processor,
    // "keep at least one non-eos token") = M / K, since M = max(2, 1 + #eos) K candidates are drawn per batch row
    const int min_keep = M / K > 1 ? M / K : 1;
    const int top_k = c->samp_top_k > 0 && c->samp_top_k < min_keep ? min_keep : c->samp_top_k;    // TopKLogitsWarper: max(top_k, min_tokens_to_keep)
    KL(KC_OTHER, 4.0 * 4 * R * V,
       launch_sample_select(lg, R, V, temperature, top_p, top_k, nullptr, nullptr, c->d_pval, c->d_pidx, c->d_probs, c->d_cand_i,
                            c->d_cand_n, c->d_zpart, c->d_spart, nullptr, c->d_bthr, nullptr, nullptr, s));
    // (the candidate lists of the nucleus search are consumed: their buffers hold the rows' min_keep best logits next)
    KL(KC_OTHER, 12.0 * R * V,
       launch_beam_sample(lg, d_run_scores, B, K, V, M, temperature, c->d_pval, c->d_bthr, min_keep, c->d_probs, c->d_cand_i, seed, step,
                          c->d_blse, d_scores, d_idx, s));
    return OPUS_OK;
}

// TopKLogitsWarper of the sampling paths of this context (opus_generate_sample, opus_debug_sample, opus_beam_sample_topk):
// k > 0 keeps the k most probable tokens (and ties with the k-th) before the nucleus; 0 = off.  transformers 4.46.3 - the
// reference's pin - defaults GenerationConfig.top_k to 50 whenever it samples; the Python mirror sets that default.
extern "C" int opus_set_sampling_top_k(opus_ctx *c, int32_t k) {
    if (!c || k < 0) return fail(OPUS_EBADARG, "set_sampling_top_k: k >= 0");
    if (k != c->samp_top_k) drop_graphs(c);                                      // the captured step holds k
    c->samp_top_k = k;
    return OPUS_OK;
}

// The truncation warpers of this context's sampling paths (opus_generate_sample, opus_generate_scored, opus_debug_sample, the
// continuous-batching session) behind top-k / top-p, in transformers' order: MinPLogitsWarper, TypicalLogitsWarper,
// EpsilonLogitsWarper, EtaLogitsWarper, min_tokens_to_keep = 1.  Off: 0, 1, 0, 0.  The captured step reads the values from device
// memory and holds only whether any warper is on.
extern "C" int opus_set_sampling_warpers(opus_ctx *c, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff) {
    if (!c) return fail(OPUS_EBADARG, "set_sampling_warpers: null context");
    if (!(min_p >= 0.f && min_p <= 1.f) || !(typical_p > 0.f && typical_p <= 1.f) || !(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f) ||
        !(eta_cutoff >= 0.f && eta_cutoff < 1.f))
        return fail(OPUS_EBADARG, "set_sampling_warpers: min_p in [0, 1], typical_p in (0, 1], epsilon_cutoff and eta_cutoff in [0, 1) "
                                  "(got %g, %g, %g, %g)", (double)min_p, (double)typical_p, (double)epsilon_cutoff, (double)eta_cutoff);
    c->h_warp = SamplingWarpers{min_p, typical_p, epsilon_cutoff, eta_cutoff};
    return OPUS_OK;
}

// KV cache rows r <- rows src[r] for every layer (Cache.reorder_cache(beam_idx) of the reference's stack: the beams that
// survive a step continue from their parents' caches).  R = the rows of the last prefill.  Two passes per layer through a
// one-layer scratch (a permutation cannot be applied in place row by row).
extern "C" int opus_kv_reorder(opus_ctx *c, const int32_t *d_src_rows, int32_t R, void *stream) {
    if (!c || !d_src_rows) return fail(OPUS_EBADARG, "kv_reorder: null pointer");
    if (!c->prefilled || R != c->cur_B) return fail(OPUS_ESHAPE, "kv_reorder: R=%d but the last prefill had %d rows", R, c->prefilled ? c->cur_B : 0);
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const opus_config &g = c->cfg;
    const size_t row = (size_t)c->cache_sb, layer = row * g.max_batch;
    if (!c->kv_tmp) HIPC(hipMalloc((void **)&c->kv_tmp, 2 * layer * sizeof(half_t)));
    c->phase = PH_DECODE;
    new_epoch(c);
    // only the filled slots (0 .. T + *step - 1, read from the device step word) of the rows that change place move
    const int nkv = g.dec_kv_heads, hd = g.dec_head_dim, T0 = c->cur_T;
    for (int l = 0; l < g.dec_layers; ++l) {
        half_t *kc = c->kc + l * c->cache_sl, *vc = c->vc + l * c->cache_sl;
        KL(KC_OTHER, 8.0 * R * nkv * hd * T0, launch_kv_gather_rows(kc, c->kv_tmp, d_src_rows, R, (int64_t)row, nkv, c->cache_sh, c->d_step, T0, hd, 0, s));
        HIPC(launch_kv_gather_rows(vc, c->kv_tmp + layer, d_src_rows, R, (int64_t)row, nkv, c->cache_sh, c->d_step, T0, hd, 0, s));
        HIPC(launch_kv_gather_rows(kc, c->kv_tmp, d_src_rows, R, (int64_t)row, nkv, c->cache_sh, c->d_step, T0, hd, 1, s));
        HIPC(launch_kv_gather_rows(vc, c->kv_tmp + layer, d_src_rows, R, (int64_t)row, nkv, c->cache_sh, c->d_step, T0, hd, 1, s));
    }
    return OPUS_OK;
}

// ------------------------------------------------------------------------------------------------ trie search
extern "C" int opus_set_trie_search(opus_ctx *c, int32_t n_states, const int32_t *edge_off, const int32_t *edge_tok,
                                    const int32_t *edge_next, int32_t n_edges, const int32_t *member, const int32_t *stop_set,
                                    int32_t n_sets, const int32_t *stop_off, const int32_t *stop_ids, void *stream) {
    const char *who = "set_trie_search";
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    if (n_states < 2 || n_edges < 1 || n_sets < 1 || !edge_off || !edge_tok || !edge_next || !member || !stop_set || !stop_off || !stop_ids)
        return fail(OPUS_EBADARG, "%s: null table or empty trie", who);
    if (n_edges >= (1 << 27)) return fail(OPUS_EBADARG, "%s: %d edges (below 2^27)", who, n_edges);
    const int V = c->cfg.dec_vocab;
    if (edge_off[0] != 0 || edge_off[1] != 0 || edge_off[n_states] != n_edges || member[0] >= 0)
        return fail(OPUS_EBADARG, "%s: edge_off must run from 0 to n_edges and state 0 is the dead state (no edges, no member)", who);
    if (stop_off[0] != 0) return fail(OPUS_EBADARG, "%s: stop_off must start at 0", who);
    for (int k = 0; k < n_sets; ++k)
        if (stop_off[k + 1] <= stop_off[k] || stop_off[k + 1] - stop_off[k] > TC_MAX_END + 1)
            return fail(OPUS_EBADARG, "%s: stop set %d holds %d ids (1 to %d)", who, k, stop_off[k + 1] - stop_off[k], TC_MAX_END + 1);
    const int n_ids = stop_off[n_sets];
    int32_t max_id = -1;
    for (int k = 0; k < n_ids; ++k) {
        if (stop_ids[k] < 0 || stop_ids[k] >= V) return fail(OPUS_EBADARG, "%s: stop id %d outside [0, %d)", who, stop_ids[k], V);
        if (stop_ids[k] > max_id) max_id = stop_ids[k];
    }
    for (int s = 0; s < n_states; ++s) {
        const int e0 = edge_off[s], e1 = edge_off[s + 1];
        if (e1 < e0 || e1 > n_edges) return fail(OPUS_EBADARG, "%s: edge_off not monotone at state %d", who, s);
        for (int e = e0; e < e1; ++e) {
            if (edge_tok[e] < 0 || edge_tok[e] >= V) return fail(OPUS_EBADARG, "%s: id %d outside [0, %d)", who, edge_tok[e], V);
            if (e > e0 && edge_tok[e] <= edge_tok[e - 1]) return fail(OPUS_EBADARG, "%s: ids of state %d not ascending", who, s);
            if (edge_next[e] < 1 || edge_next[e] >= n_states) return fail(OPUS_EBADARG, "%s: target %d outside [1, %d)", who, edge_next[e], n_states);
        }
        if (e1 > e0 && edge_tok[e1 - 1] > max_id) max_id = edge_tok[e1 - 1];
        if (stop_set[s] < 0 || stop_set[s] >= n_sets) return fail(OPUS_EBADARG, "%s: stop set %d of state %d outside [0, %d)", who, stop_set[s], s, n_sets);
    }
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t o_tok = align_up((size_t)(n_states + 1) * 4), o_nxt = o_tok + align_up((size_t)n_edges * 4),
                 o_mem = o_nxt + align_up((size_t)n_edges * 4), o_set = o_mem + align_up((size_t)n_states * 4),
                 o_off = o_set + align_up((size_t)n_states * 4), o_ids = o_off + align_up((size_t)(n_sets + 1) * 4),
                 total = o_ids + align_up((size_t)n_ids * 4);
    HIPC(hipStreamSynchronize(s));           // a call in flight may still read the table that is replaced
    c->ts.edge_off = nullptr;
    if (total > c->ts_tab_bytes) {
        if (c->ts_tab) HIPC(hipFree(c->ts_tab));
        c->ts_tab = nullptr;
        c->ts_tab_bytes = 0;
        HIPC(hipMalloc((void **)&c->ts_tab, total));
        c->ts_tab_bytes = total;
    }
    char *t = c->ts_tab;
    HIPC(hipMemcpyAsync(t, edge_off, (size_t)(n_states + 1) * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_tok, edge_tok, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_nxt, edge_next, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_mem, member, (size_t)n_states * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_set, stop_set, (size_t)n_states * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_off, stop_off, (size_t)(n_sets + 1) * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(t + o_ids, stop_ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, s));
    HIPC(hipStreamSynchronize(s));           // the host arrays are the caller's again
    auto at = [&](size_t o) { return reinterpret_cast<const int32_t *>(t + o); };
    c->ts = TrieSearchTable{at(0), at(o_tok), at(o_nxt), at(o_mem), at(o_set), at(o_off), at(o_ids), n_states, n_edges};
    c->ts_max_id = max_id;
    return OPUS_OK;
}

extern "C" int opus_trie_search_begin(opus_ctx *c, const float *d_last_rows, int32_t P, void *stream) {
    OPC(need_ready(c));
    if (!d_last_rows) return fail(OPUS_EBADARG, "trie_search_begin: null pointer");
    if (P < 1 || P > c->cfg.max_batch) return fail(OPUS_ESHAPE, "trie_search_begin: P=%d prompts, the context holds max_batch=%d", P, c->cfg.max_batch);
    hipStream_t s = (hipStream_t)stream;
    new_epoch(c);                            // (d_xl and the logits are the decode state's)
    c->prefilled = false;
    c->cur_B = 0;
    c->phase = PH_DECODE;
    HIPC(hipMemcpyAsync(c->d_xl, d_last_rows, (size_t)P * c->cfg.dec_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (c->cfg.dec_arch == 1) return lm_head_opt(c, s, P);
    ResidShadow none;
    return lm_head(c, s, none, P);
}

// the level on `logits` (rows of V floats): the rows' log-sum-exp (the arg-max pass of opus_debug_argmax_lse; its indices land in
// d_tok, which the level overwrites), then trie_beam_expand_kernel
static int trie_search_level(opus_ctx *c, const char *who, const float *logits, int V, const opus_trie_search_io *io, bool first, hipStream_t s) {
    if (!c->ts.edge_off) return fail(OPUS_ESTATE, "%s: no table set (opus_set_trie_search)", who);
    if (!io || !io->d_state || !io->d_score || !io->d_tok || !io->d_parent || !io->d_pool_member || !io->d_pool_lp || !io->d_pool_stop ||
        !io->d_flags || !io->d_words || !io->d_lse)
        return fail(OPUS_EBADARG, "%s: null pointer", who);
    if (io->P < 1 || io->K < 1 || io->K > TS_MAXK || io->top < 1 || io->top > io->K || (int64_t)io->P * io->K > c->cfg.max_batch)
        return fail(OPUS_ESHAPE, "%s: P=%d K=%d top=%d (1 <= top <= K <= %d, P x K <= max_batch=%d)", who, io->P, io->K, io->top, TS_MAXK, c->cfg.max_batch);
    if (c->ts_max_id >= V) return fail(OPUS_ESHAPE, "%s: the table holds id %d, V=%d", who, c->ts_max_id, V);
    OPC(ensure_gen_mem(c));
    const int rows = first ? io->P : io->P * io->K;
    KL(KC_OTHER, 4.0 * rows * V, launch_argmax_lse_partial(logits, rows, V, c->d_pval, c->d_pidx, c->d_gpsum, s));
    KL(KC_OTHER, 512.0 * rows, launch_argmax_lse_final(c->d_pval, c->d_pidx, c->d_gpsum, rows, io->d_tok, io->d_lse, s));
    TrieSearchLevel a{};
    a.logits = logits; a.lse = io->d_lse; a.ld = V;
    a.K = io->K; a.top = io->top; a.include_stop = io->include_stop ? 1 : 0; a.rows_per_prompt = first ? 1 : io->K;
    a.state_in = io->d_state; a.score_in = io->d_score;
    a.tok = io->d_tok; a.parent = io->d_parent; a.state_out = io->d_state; a.score_out = io->d_score;
    a.pool_member = io->d_pool_member; a.pool_lp = io->d_pool_lp; a.pool_stop = io->d_pool_stop;
    a.flags = io->d_flags; a.edge_lp = io->d_edge_lp; a.beam_stop = io->d_beam_stop;
    // (bytes: per beam a few hundred edges' ids, targets, member words and logits; counted for the widest case the table allows)
    KL(KC_TRIE_SEARCH, 16.0 * io->P * io->K * (double)c->ts.n_edges / (double)c->ts.n_states, launch_trie_beam_expand(c->ts, a, io->P, io->d_words, s));
    return OPUS_OK;
}

extern "C" int opus_trie_search_level(opus_ctx *c, const opus_trie_search_io *io, int32_t first, void *stream) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    HIPC(hipSetDevice(c->device));
    if (!first && !c->prefilled) return fail(OPUS_ESTATE, "trie_search_level before the beams' prefill");
    if (io && !first && io->P * io->K != c->cur_B)
        return fail(OPUS_ESHAPE, "trie_search_level: P=%d x K=%d rows, the last step had %d", io->P, io->K, c->cur_B);
    c->phase = PH_DECODE;
    return trie_search_level(c, "trie_search_level", c->d_logits, c->cfg.dec_vocab, io, first != 0, (hipStream_t)stream);
}

extern "C" int opus_debug_trie_beam_expand(opus_ctx *c, const float *d_logits, int32_t V, const opus_trie_search_io *io, int32_t first,
                                           void *stream) {
    if (!c || !d_logits) return fail(OPUS_EBADARG, "debug_trie_beam_expand: null pointer");
    if (V < 1) return fail(OPUS_ESHAPE, "debug_trie_beam_expand: V=%d", V);
    HIPC(hipSetDevice(c->device));
    c->phase = PH_OTHER;
    return trie_search_level(c, "debug_trie_beam_expand", d_logits, V, io, first != 0, (hipStream_t)stream);
}

// fp32 logits [B, dec_vocab] of the most recent prefill / decode step of this context (the optional logits gather of
// SURVEY 8e; also what a caller needs to apply its own logits processors).
extern "C" int opus_last_logits(opus_ctx *c, float *d_out, int32_t B, void *stream) {
    if (!c || !d_out) return fail(OPUS_EBADARG, "last_logits: null pointer");
    if (!c->prefilled) return fail(OPUS_ESTATE, "last_logits before prefill");
    if (B < 1 || B > c->cur_B) return fail(OPUS_ESHAPE, "last_logits: B=%d but the last prefill had %d rows", B, c->cur_B);
    HIPC(hipSetDevice(c->device));
    HIPC(hipMemcpyAsync(d_out, c->d_logits, (size_t)B * c->cfg.dec_vocab * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return OPUS_OK;
}

extern "C" int opus_debug_attention(opus_ctx *c, const void *Q, const void *K, const void *V, void *O,
                                    const int32_t *kstart, const int32_t *kend, int32_t B, int32_t T, int32_t heads,
                                    int32_t group, int32_t hd, int32_t causal, float scale, void *stream) {
    if (!c || !Q || !K || !V || !O) return fail(OPUS_EBADARG, "debug_attention: null pointer");
    if (B < 1 || T < 1 || heads < 1 || group < 1 || heads % group) return fail(OPUS_ESHAPE, "debug_attention: shape");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    AttnParams a;
    const int kvh = heads / group;
    a.Q = (const half_t *)Q; a.K = (const half_t *)K; a.V = (const half_t *)V; a.O = (half_t *)O;
    a.q_st = (int64_t)heads * hd; a.q_sb = a.q_st * T;
    a.k_st = a.v_st = (int64_t)kvh * hd; a.k_sb = a.v_sb = a.k_st * T;
    a.o_st = a.q_st; a.o_sb = a.q_sb;
    a.kstart = kstart; a.kend = kend; a.B = B; a.T = T; a.heads = heads; a.group = group; a.head_dim = hd;
    a.causal = causal; a.scale = scale;
    KLF(KC_ATTN_PREFILL, 2.0 * B * T * hd * (2.0 * heads + 2.0 * kvh), (causal ? 2.0 : 4.0) * B * (double)T * T * heads * hd,
        launch_attn_prefill(a, s));
    return OPUS_OK;
}

// attn_prefill_kernel launched as the product launches it: the caller's pointers and strides go into AttnParams as they stand
// (the encoder's [rows, 3 D] buffer, the decoder's [rows, (nh + 2 nkv) hd] one), token-packed (d_cu) with or without q_trim, or
// padded with d_kstart / d_kend.  No buffer of the context is touched.  *qt_used (HOST) = the query tiles per wave the launcher
// took (0 when nothing was launched).
extern "C" int opus_debug_attn_prefill(opus_ctx *c, const void *Q, const void *K, const void *V, void *O, int64_t q_st, int64_t k_st,
                                       int64_t v_st, int64_t o_st, int64_t q_sb, int64_t k_sb, int64_t v_sb, int64_t o_sb,
                                       const int32_t *kstart, const int32_t *kend, const int32_t *cu, int32_t B, int32_t T,
                                       int32_t heads, int32_t group, int32_t hd, int32_t causal, int32_t q_trim, float scale,
                                       int32_t *qt_used, void *stream) {
    if (qt_used) *qt_used = 0;
    if (!c || !Q || !K || !V || !O || !qt_used) return fail(OPUS_EBADARG, "debug_attn_prefill: null pointer");
    if (B < 1 || T < 1 || heads < 1 || group < 1 || heads % group || hd < 1) return fail(OPUS_ESHAPE, "debug_attn_prefill: shape");
    if (q_st < 1 || k_st < 1 || v_st < 1 || o_st < 1) return fail(OPUS_ESHAPE, "debug_attn_prefill: token strides must be positive");
    if (causal && cu) return fail(OPUS_EUNSUPPORTED, "debug_attn_prefill: no causal token-packed form");
    if (q_trim && (!cu || T <= 2)) return fail(OPUS_ESHAPE, "debug_attn_prefill: q_trim needs cu and T > 2");
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    AttnParams a;
    a.Q = (const half_t *)Q; a.K = (const half_t *)K; a.V = (const half_t *)V; a.O = (half_t *)O;
    a.q_st = q_st; a.k_st = k_st; a.v_st = v_st; a.o_st = o_st;
    a.q_sb = cu ? 0 : q_sb; a.k_sb = cu ? 0 : k_sb; a.v_sb = cu ? 0 : v_sb; a.o_sb = cu ? 0 : o_sb;
    a.kstart = kstart; a.kend = kend; a.cu = cu; a.q_trim = q_trim ? 1 : 0;
    a.B = B; a.T = T; a.heads = heads; a.group = group; a.head_dim = hd; a.causal = causal ? 1 : 0; a.scale = scale;
    const int kvh = heads / group;
    KLF(KC_ATTN_PREFILL, 2.0 * B * T * hd * (2.0 * heads + 2.0 * kvh), (causal ? 2.0 : 4.0) * B * (double)T * T * heads * hd,
        launch_attn_prefill(a, s));
    *qt_used = attn_prefill_query_tiles(a);
    return OPUS_OK;
}

// The input of one debug launch of attn_decode_kernel: finished projections (qkv) or the fused form the decode step takes at
// 4 < B <= 64 (raw k-part slabs + the sums of squares of the GEMM's input rows + an optional bias), the caller's pointers as they stand
struct DecodeForm {
    const void *qkv = nullptr;
    const float *slabs = nullptr, *row_ssq = nullptr, *bias = nullptr;
    int ks = 0, row_nblk = 0, K = 0, out_tiled = 0;
    float eps = 0.f;
    void *k_cache = nullptr, *v_cache = nullptr;      // (optional) layer 0's whole cache afterwards [B, kv, ctx_cap, hd]
    int32_t *gp_used = nullptr;                       // (optional, host) query heads per workgroup of the launch
};
// the range checks both decode debug entries share (before any device call)
static int debug_attn_decode_check(opus_ctx *c, const char *who, const void *d_k_hist, const void *d_v_hist, int B, int T0, int step) {
    const opus_config &g = c->cfg;
    if (B < 1 || B > g.max_batch || T0 < 1 || T0 > g.max_prompt || step < 0 || step >= g.max_new_tokens)
        return fail(OPUS_ESHAPE, "%s: B=%d T0=%d step=%d exceed the context (%d, %d, %d)", who, B, T0, step, g.max_batch,
                    g.max_prompt, g.max_new_tokens);
    if (T0 + step > 0 && (!d_k_hist || !d_v_hist)) return fail(OPUS_EBADARG, "%s: history is null", who);
    return OPUS_OK;
}
// layer 0 of the cache <- the history, the step word, kstart[] and the rotary rows of the step as the embedding kernel sets them,
// then ONE launch of attn_decode_kernel with the parameters attn_decode() gives it for this input form
static int debug_attn_decode_launch(opus_ctx *c, const DecodeForm &f, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                                    int B, int T0, int step, void *d_out, void *d_k_new, void *d_v_new, void *stream) {
    const opus_config &g = c->cfg;
    const int L = T0 + step, nkv = g.dec_kv_heads, hd = g.dec_head_dim, ctx_cap = g.max_prompt + g.max_new_tokens;
    HIPC(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t pitch = (size_t)c->cache_sh * sizeof(half_t);
    OPC(seed_cache(c, s, d_k_hist, d_v_hist, d_kstart, B, L));
    OPC(reset_step(c, s, T0, step));
    // (the embedding kernel with a zero-width row: only its rotary-row part runs)
    HIPC(launch_embed_tokens(c->d_next, nullptr, B, 0, 1, c->d_xl, nullptr, nullptr, 0, c->cs_dec, c->d_kstart, c->d_step, -1, hd / 2,
                             c->cs_row, nullptr, 0, s));
    AttnDecodeParams a;
    a.qkv = (const half_t *)f.qkv; a.slabs = nullptr; a.ks = 0; a.slab_stride = 0; a.row_ssq = nullptr; a.row_nblk = 0; a.eps = 0.f; a.K = 0;
    a.bias = nullptr;
    if (f.slabs) {
        a.qkv = nullptr; a.slabs = f.slabs; a.ks = f.ks; a.slab_stride = (int64_t)B * (g.dec_heads + 2 * nkv) * hd;
        a.row_ssq = f.row_ssq; a.row_nblk = f.row_nblk; a.eps = f.eps; a.K = f.K; a.bias = f.bias;
    }
    a.cs_row = c->cs_row; a.kstart = c->d_kstart; a.step = c->d_step; a.T0 = -1; a.nh = g.dec_heads; a.nkv = nkv;
    a.kc = c->kc; a.vc = c->vc; a.cache_sb = c->cache_sb; a.cache_sh = c->cache_sh;
    a.ctx_cap = ctx_cap; a.scale = 1.0f / sqrtf((float)hd); a.out = (half_t *)d_out; a.out_tiled = f.out_tiled;
    c->phase = PH_DECODE;
    KL(KC_ATTN_DECODE, 4.0 * B * nkv * hd * (L + 1), launch_attn_decode(a, B, hd, s));
    if (f.gp_used) *f.gp_used = attn_decode_group(B, g.dec_heads, nkv);
    const size_t one = (size_t)hd * sizeof(half_t);
    if (d_k_new) HIPC(hipMemcpy2DAsync(d_k_new, one, c->kc + (size_t)L * hd, pitch, one, (size_t)B * nkv, hipMemcpyDeviceToDevice, s));
    if (d_v_new) HIPC(hipMemcpy2DAsync(d_v_new, one, c->vc + (size_t)L * hd, pitch, one, (size_t)B * nkv, hipMemcpyDeviceToDevice, s));
    const size_t all = (size_t)ctx_cap * hd * sizeof(half_t);
    if (f.k_cache) HIPC(hipMemcpy2DAsync(f.k_cache, all, c->kc, pitch, all, (size_t)B * nkv, hipMemcpyDeviceToDevice, s));
    if (f.v_cache) HIPC(hipMemcpy2DAsync(f.v_cache, all, c->vc, pitch, all, (size_t)B * nkv, hipMemcpyDeviceToDevice, s));
    c->prefilled = false;                                     // (the cache no longer belongs to a prefill)
    new_epoch(c);
    return OPUS_OK;
}

// attn_decode_kernel exactly as decode_step() launches it (finished fp16 projections in, no k-part slabs), on layer 0 of this
// context's KV cache: the history d_k_hist / d_v_hist fp16 [B, kv heads, L, hd] (keys already rotated, as the cache holds them)
// is copied into slots 0 .. L-1 (L = T0 + step), the step word, kstart[] and the rotary rows of the step are set as the
// embedding kernel sets them, then ONE launch: rotary(q, k) at position L - kstart[b], append at slot L, softmax over the
// slots kstart[b] .. L.  d_out fp16 [B, heads hd]; d_k_new / d_v_new (optional) fp16 [B, kv heads, hd] = what slot L holds
// afterwards.  The kernel-level parity test of the key-tile loop (tests/test_gpu_longctx.py): rows D3 / D4.
extern "C" int opus_debug_attn_decode(opus_ctx *c, const void *d_qkv, const void *d_k_hist, const void *d_v_hist,
                                      const int32_t *d_kstart, int32_t B, int32_t T0, int32_t step, void *d_out, void *d_k_new,
                                      void *d_v_new, void *stream) {
    if (!c || !d_qkv || !d_kstart || !d_out) return fail(OPUS_EBADARG, "debug_attn_decode: null pointer");
    OPC(debug_attn_decode_check(c, "debug_attn_decode", d_k_hist, d_v_hist, B, T0, step));
    DecodeForm f;
    f.qkv = d_qkv;
    return debug_attn_decode_launch(c, f, d_k_hist, d_v_hist, d_kstart, B, T0, step, d_out, d_k_new, d_v_new, stream);
}

// The same launch in every form the product takes (tests/test_gpu_attn_decode.py): the input either finished projections
// (d_qkv) or, as decode_step() at 4 < B <= 64, d_slabs fp32 [ks, B, (heads + 2 kv) hd] raw k-part slabs with d_row_ssq fp32
// [B, row_nblk] (the sums of squares of the GEMM's input rows over K columns), eps and an optional d_bias fp32 - summed, scaled
// by rsqrt(sum / K + eps), biased and rounded by the attention kernel itself; the output row-major or fragment-ordered
// (out_tiled: 16 ceil(B / 16) rows at tiled_off).  d_k_cache / d_v_cache (optional) [B, kv heads, max_prompt + max_new_tokens,
// hd]: layer 0's cache after the launch.  *gp_used (HOST) = the query heads per workgroup the launcher took, 0 when nothing
// was launched.  Every refusal comes before the first device call.
extern "C" int opus_debug_attn_decode_form(opus_ctx *c, const void *d_qkv, const float *d_slabs, int32_t ks, const float *d_row_ssq,
                                           int32_t row_nblk, int32_t K, float eps, const float *d_bias, const void *d_k_hist,
                                           const void *d_v_hist, const int32_t *d_kstart, int32_t B, int32_t T0, int32_t step,
                                           int32_t out_tiled, void *d_out, void *d_k_new, void *d_v_new, void *d_k_cache,
                                           void *d_v_cache, int32_t *gp_used, void *stream) {
    if (gp_used) *gp_used = 0;
    if (!c || !d_kstart || !d_out || !gp_used) return fail(OPUS_EBADARG, "debug_attn_decode_form: null pointer");
    if ((d_qkv != nullptr) == (d_slabs != nullptr))
        return fail(OPUS_EBADARG, "debug_attn_decode_form: exactly one of d_qkv and d_slabs must be given");
    OPC(debug_attn_decode_check(c, "debug_attn_decode_form", d_k_hist, d_v_hist, B, T0, step));
    if (d_slabs) {
        if (ks < 1 || ks > 8) return fail(OPUS_ESHAPE, "debug_attn_decode_form: ks=%d outside 1 .. 8", ks);
        if (row_nblk < 1 || K < 1) return fail(OPUS_ESHAPE, "debug_attn_decode_form: row_nblk=%d K=%d must be positive", row_nblk, K);
        if (!d_row_ssq) return fail(OPUS_ESHAPE, "debug_attn_decode_form: slabs come with the rows' sums of squares (d_row_ssq)");
    }
    if (out_tiled && (int64_t)c->cfg.dec_heads * c->cfg.dec_head_dim % 64)
        return fail(OPUS_ESHAPE, "debug_attn_decode_form: out_tiled needs heads * head_dim = %d to be a multiple of 64",
                    c->cfg.dec_heads * c->cfg.dec_head_dim);
    DecodeForm f;
    f.qkv = d_qkv; f.slabs = d_slabs; f.row_ssq = d_row_ssq; f.bias = d_slabs ? d_bias : nullptr;
    f.ks = ks; f.row_nblk = row_nblk; f.K = K; f.eps = eps; f.out_tiled = out_tiled ? 1 : 0;
    f.k_cache = d_k_cache; f.v_cache = d_v_cache; f.gp_used = gp_used;
    return debug_attn_decode_launch(c, f, d_k_hist, d_v_hist, d_kstart, B, T0, step, d_out, d_k_new, d_v_new, stream);
}

// Run-time tuning knobs (A/B aids of the benchmarks and tests; process-wide): "no_stream", "pp_gm", "misc0" .. "misc7".
extern "C" int opus_debug_knob(opus_ctx *c, const char *name, int32_t value) {
    if (!name) return fail(OPUS_EBADARG, "debug_knob: null name");
    if (c) drop_graphs(c);   // a captured decode graph replays the kernels it was recorded with
    if (!strcmp(name, "no_stream")) g_knobs.no_stream = value;
    else if (!strcmp(name, "debug_a_tiled")) g_knobs.debug_a_tiled = value;
    else if (!strcmp(name, "no_ln_fusion")) g_knobs.no_ln_fusion = value;
    else if (!strcmp(name, "enc_full_last_layer")) g_knobs.enc_full_last_layer = value;
    else if (!strcmp(name, "poison_handoff")) {   // test aid: what an aborted launch leaves behind - every ticket drawn once, no flag set
        if (!c) return fail(OPUS_EBADARG, "poison_handoff needs a context");
        std::vector<int32_t> h(HANDOFF_ERR, 0);
        // (a ticket count alone cannot tell "one stale ticket + three arrivals" from four arrivals: detection is certain only for
        //  values no clean launch can reach - value > 1 writes that into the tickets -; the cure is the per-call zeroing)
        if (value) for (int i = 0; i < HANDOFF_ERR; ++i) h[i] = i < 512 ? value : ((i & 1) ? 0 : 1);
        HIPC(hipSetDevice(c->device));
        HIPC(hipDeviceSynchronize());
        HIPC(hipMemcpy(c->d_cnt, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    else if (!strcmp(name, "pp_gm")) { if (value < 1 || value > 64) return fail(OPUS_EBADARG, "pp_gm out of range"); g_knobs.pp_gm = value; }
    else if (!strncmp(name, "misc", 4) && name[4] >= '0' && name[4] <= '7' && !name[5]) g_knobs.misc[name[4] - '0'] = value;
    else return fail(OPUS_EBADARG, "debug_knob: unknown knob '%s'", name);
    return OPUS_OK;
}

// Counters of this context (no reference counterpart): "graph_instantiations" = decode-step hipGraphs instantiated since the
// context was created (one per distinct batch size / token budget / sampling setting, none per prompt length);
// "graph_replays" = decode steps launched from a graph; "graphs_cached"; "decode_steps" = decode steps opus_generate_* enqueued
// (with an EOS id or a stop sequence: at most 2 past the step at which the last row finished).  Unknown name / null: -1.
extern "C" int64_t opus_stat(opus_ctx *c, const char *name) {
    if (!c || !name) return -1;
    if (!strcmp(name, "graph_instantiations")) return c->graph_instantiations;
    if (!strcmp(name, "graph_replays")) return c->graph_replays;
    if (!strcmp(name, "graphs_cached")) return (int64_t)c->graphs.size();
    if (!strcmp(name, "decode_steps")) return c->decode_steps;
    if (!strcmp(name, "w8_gemms")) return c->wq_gemms[WQ_FP8];
    if (!strcmp(name, "w4_gemms")) return c->wq_gemms[WQ_MXFP4];
    if (!strcmp(name, "prefills_behind")) return c->prefills_behind;
    if (!strcmp(name, "stream_steps")) return c->stream_steps;
    if (!strcmp(name, "stream_refills")) return c->stream_refills;
    if (!strcmp(name, "stream_graph")) return c->stream_graph.exec ? 1 : 0;
    if (!strcmp(name, "lookup_passes")) return c->lookup_passes;
    if (!strcmp(name, "cache_epoch")) return c->epoch;       // (what opus_llama_prefix_export takes, also behind a generate call)
    return -1;
}

// ------------------------------------------------------------------------------------------------ timing
extern "C" int opus_timing_enable(opus_ctx *c, int32_t on) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    c->timing = on != 0;
    return OPUS_OK;
}
extern "C" int opus_timing_reset(opus_ctx *c) {
    if (!c) return fail(OPUS_EBADARG, "ctx is null");
    HIPC(hipDeviceSynchronize());
    timing_clear(c);
    return OPUS_OK;
}
static const char *kclass_names[KC_COUNT] = {"gemm_skinny", "gemm_mid", "gemm_wide", "gemm_ring", "gemm_pp", "gemm_tile", "splitk_reduce",
                                            "attn_prefill", "attn_decode", "norm", "other", "gemm_stream", "contact", "trie_search", "topk", "constraint", "guidance", "mlm", "logitproc",
                                            "xent"};
static const char *phase_names[PH_COUNT] = {"encode", "project", "splice", "prefill", "decode", "other", "score"};

extern "C" int opus_timing_get(opus_ctx *c, const char *kernel_class, const char *phase, double *ms, int64_t *launches,
                               double *bytes, double *flops) {
    if (!c || !kernel_class || !phase || !ms || !launches || !bytes || !flops) return fail(OPUS_EBADARG, "null argument");
    int k = -1, ph = -1;
    const bool any_k = !strcmp(kernel_class, "*"), any_p = !strcmp(phase, "*");
    for (int i = 0; i < KC_COUNT; ++i) if (!strcmp(kclass_names[i], kernel_class)) k = i;
    for (int i = 0; i < PH_COUNT; ++i) if (!strcmp(phase_names[i], phase)) ph = i;
    if (k < 0 && !any_k) return fail(OPUS_EBADARG, "unknown kernel class '%s'", kernel_class);
    if (ph < 0 && !any_p) return fail(OPUS_EBADARG, "unknown phase '%s'", phase);
    HIPC(hipDeviceSynchronize());
    double t = 0, b = 0, f = 0;
    int64_t n = 0;
    for (auto &r : c->recs) {
        if ((!any_k && r.klass != k) || (!any_p && r.phase != ph)) continue;
        float e = 0;
        HIPC(hipEventElapsedTime(&e, r.e0, r.e1));
        t += e;
        b += r.bytes;
        f += r.flops;
        ++n;
    }
    *ms = t;
    *launches = n;
    *bytes = b;
    *flops = f;
    return OPUS_OK;
}

extern "C" int opus_timing_names(char *buf, int32_t cap) {
    if (!buf || cap < 1) return fail(OPUS_EBADARG, "null buffer");
    std::string out;
    for (int i = 0; i < KC_COUNT; ++i) { out += kclass_names[i]; out += i + 1 < KC_COUNT ? "," : ";"; }
    for (int i = 0; i < PH_COUNT; ++i) { out += phase_names[i]; if (i + 1 < PH_COUNT) out += ","; }
    if ((int)out.size() + 1 > cap) return fail(OPUS_ESHAPE, "buffer too small (%zu needed)", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return OPUS_OK;
}
