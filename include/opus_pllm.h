/*
 * opus_pllm.h - C ABI of the MI355X-native multi_modality_v1 inference path (libopus_pllm.so).
 *
 * The reference (Fanchuana/OPUS-PLLM) has no plugin / FFI interface: its boundary is the Python call
 * surface used by the eval scripts.  This header is the boundary a binding for that surface
 * uses; every entry point cites the reference code it replaces.  The Python shim in
 * opus-pllm_amd/_cabi.py binds exactly these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - extern "C", plain C types, opaque opus_ctx*; no C++ exception crosses the boundary.
 *   - Every function returns 0 (OPUS_OK) or a negative error class; the message is available from
 *     opus_last_error() (thread-local).
 *   - All pointers named d_* are DEVICE pointers owned by the caller (PyTorch keeps ownership and
 *     lifetime of weights and I/O buffers); the library owns only the context, its workspace and
 *     its KV cache, all sized at opus_ctx_create from the config's capacity fields.
 *   - All work is ordered on the caller's hipStream_t (passed as void*; NULL = default stream).
 *     No hidden device synchronisation, except where a function returns a HOST scalar that depends
 *     on device data (documented per function: it synchronises the given stream once).
 *   - A context is bound to one device and is not thread-safe: one host thread drives a context at a time.  A process may
 *     hold several contexts on the same device that BIND THE SAME weight pointers (read-only; each context owns its workspace,
 *     KV cache, decode graph and hand-off words): two batches in flight per GPU (`model.new_context()`, one host thread and one
 *     stream per context).  One process per GPU as in the reference (model/builder.py:41).
 *   - Kernels that combine split-K parts INSIDE one launch wait only for workgroups that are already running, with a bounded
 *     wait; a wait that runs out (ticket words poisoned by an aborted launch) sets a device error word instead of hanging, which
 *     the next call that synchronises (opus_generate_*, opus_check_error) returns as OPUS_EHIP.  The words are re-zeroed at
 *     the head of every encode / projector / prefill / decode step.
 */
#ifndef OPUS_PLLM_H
#define OPUS_PLLM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPUS_ABI_VERSION 10

enum opus_status {
    OPUS_OK = 0,
    OPUS_EBADARG = -1,      /* null pointer, bad enum, negative size */
    OPUS_ESHAPE = -2,       /* shape exceeds the context capacity or violates a kernel granule */
    OPUS_EHIP = -3,         /* a HIP runtime call failed */
    OPUS_ERCCL = -4,        /* reserved: collective failure */
    OPUS_EUNSUPPORTED = -5, /* valid request the build does not implement */
    OPUS_ESTATE = -6        /* missing weights / call out of order */
};

/* OPUS_F8E4M3 (OCP e4m3fn codes) and OPUS_I8: the FP8 form of the decoder-layer weights only (opus_quantize_fp8); added within
 * ABI 10 (new values only). */
/* OPUS_F4E2M1X2 (two OCP e2m1 codes per byte, the lower k in the low nibble) and OPUS_E8M0 (power-of-two scale bytes): the MXFP4
 * form of the decoder-layer weights only (opus_quantize_mxfp4); added within ABI 10 (new values only). */
enum opus_dtype { OPUS_F16 = 0, OPUS_F32 = 1, OPUS_I32 = 2, OPUS_I64 = 3, OPUS_U8 = 4, OPUS_F8E4M3 = 5, OPUS_I8 = 6,
                  OPUS_F4E2M1X2 = 7, OPUS_E8M0 = 8 };

/* Shapes of the path.  The reference hard-codes or threads these through a global class
 * (model/builder.py:24-28, protein_projector/builder.py:7-13, protein_mlp/builder.py:11-15,
 * cstp_v3/modelling.py:21); here they are explicit.  Field order == opus-pllm_amd/config.py. */
typedef struct opus_config {
    int32_t enc_layers, enc_dim, enc_heads, enc_ffn, enc_vocab;
    float enc_ln_eps, enc_rope_theta;
    int32_t has_protein_projector, proj_dim, n_prot_tokens, switch_depth;
    int32_t dec_layers, dec_dim, dec_heads, dec_kv_heads, dec_head_dim, dec_ffn, dec_vocab;
    float dec_rms_eps, dec_rope_theta;
    int32_t max_batch, max_enc_tokens, max_prompt, max_new_tokens;
    /* decoder family (model/builder.py:60-92): dec_arch 0 = Llama / Qwen2 (dec_qkv_bias: q/k/v biases),
     * 1 = OPT / Galactica with do_layer_norm_before (learned positions [dec_max_pos + 2, dim], LayerNorm, biased
     * projections, fc1 - activation - fc2; dec_act 0 = GELU (Galactica), 1 = ReLU (facebook/opt-*); dec_rms_eps is then the LayerNorm epsilon) */
    int32_t dec_arch, dec_qkv_bias, dec_act, dec_max_pos;
} opus_config;

typedef struct opus_ctx opus_ctx;

int opus_abi_version(void);
/* The 16-bit operand type of THIS build of the library: 0 = IEEE fp16 (libopus_pllm.so: the reference's unquantised dtype,
 * model/builder.py:57 `torch_dtype=torch.float16`), 1 = bfloat16 (libopus_pllm_bf16.so, built from the same sources with
 * -DOPUS_BF16: SURVEY 8(d) "bf16 switchable").  Wherever this header says "fp16" for a matrix, an activation or the KV cache it
 * means this type (dtype tag OPUS_F16 = "the build's 16-bit type"); accumulation, residual stream, norms, softmax and logits
 * are fp32 in both builds. */
int opus_operand_dtype(void);
const char *opus_last_error(void);

/* Bytes of device memory opus_ctx_create will allocate for this config (workspace + KV cache). */
int64_t opus_workspace_bytes(const opus_config *cfg);

/* Replaces the module construction of load_pretrained_model / initialize_protein_modules
 * (model/builder.py:29-131, model/opus_arch.py:46-90): creates the per-process context on `device`. */
int opus_ctx_create(const opus_config *cfg, int device, opus_ctx **out);
int opus_ctx_destroy(opus_ctx *ctx);

/* Bind one weight tensor (borrowed device pointer).  Names and layouts: DESIGN.md "Weights in HBM"
 * (fused [q;k;v] rows, gate/up interleaved in 16-row groups, RMSNorm weights folded, panel-tiled).  Replaces the state-dict loads of
 * model/builder.py:60-65,107-111 and opus_arch.py:81-90.  fp16 for matrices, fp32 for vectors. */
int opus_bind_weight(opus_ctx *ctx, const char *name, const void *d_ptr, int dtype, int ndim,
                     const int64_t *shape);
/* 0 when every tensor the config requires is bound; otherwise OPUS_ESTATE and the first missing
 * name in opus_last_error(). */
int opus_weights_ready(opus_ctx *ctx);

/* Row L1: PeftModel.merge_and_unload (model/builder.py:107-109): W[out,in] += scale * B[out,r] A[r,in],
 * fp16 weights, fp32 accumulation, in place. */
int opus_lora_merge(void *d_W, const void *d_A, const void *d_B, float scale, int64_t out_f, int64_t in_f,
                    int32_t r, void *stream);

/* Deterministic synthetic tensor fill (no checkpoints exist offline; opus-pllm_amd/synth.py is the
 * NumPy twin, bit-identical).  Element (row, col) of the LOGICAL [rows, cols] tensor goes to dst row
 * (row / row_block) * row_stride + row_off + row % row_block; tiled != 0 writes the panel-tiled GEMM
 * weight layout (DESIGN.md "Weights in HBM"); fold_std/fold_mean != 0 multiplies column k by element k
 * of the synthetic vector (fold_seed, fold_std, fold_mean): an RMSNorm weight folded into the
 * projection that consumes the normalised activations. */
int opus_fill_synth(void *d_dst, int dtype, int64_t rows, int64_t cols, uint64_t tensor_seed, float std,
                    float mean, int64_t row_block, int64_t row_stride, int64_t row_off, int32_t tiled,
                    uint64_t fold_seed, float fold_std, float fold_mean, void *stream);

/* Load-time re-layout of one GEMM weight: row-major fp16 W[N,K] (nn.Linear layout) -> the panel-tiled
 * layout the kernels stream (16-row x 64-k blocks in MFMA B-fragment order).  N % 16 == 0, K % 64 == 0. */
int opus_tile_weight(const void *d_src, void *d_dst, int64_t N, int64_t K, void *stream);

/* FP8 decoder weights (a decode-throughput option, not a capacity one: the fp16 tensors stay bound).  Quantises one decoder-layer
 * weight after all load-time fusion and before tiling: row-major W[N,K] in the operand type (N % 16 == 0, K % 64 == 0) ->
 *   d_e8  int8 [N]     e_n = the smallest integer with absmax_n 2^-e_n <= 448 (0 for an all-zero row; never below -120)
 *   d_q8  N K bytes    OCP e4m3fn codes q = RNE(W 2^-e_n) in FP8 panels: block (p = n / 16, c = k / 64) is the 1 KB at
 *                      ((p K / 64) + c) 1024; lane g 16 + li (n = 16 p + li) owns 16 bytes, bytes 0..7 = k 64 c + 8 g + j,
 *                      bytes 8..15 = k 64 c + 32 + 8 g + j.  No code is NaN; a code whose value q 2^e_n would be subnormal in the
 *                      operand type is +0; a code that rounding carried past the operand type's largest finite value is the next
 *                      code towards zero
 *   d_dq  (optional)   q 2^e_n in the operand type, row-major [N,K], exact; may be d_src (in place)
 * Bind q8 / e8 as "dec.{l}.{wqkv,wo,wgu,wd}.q8" (OPUS_F8E4M3 [N,K]) / ".e8" (OPUS_I8 [N]) beside the panel-tiled dq bound under the
 * usual name (Llama / Qwen2 layers; both tensors of a projection or neither): the decode step's GEMMs that have an FP8 form (the
 * weight-streaming kernels: skinny at 1 .. 4 rows; stream, wide and mid at 5 .. 64 rows) then stream half the bytes of the same numbers; every other launch reads the fp16 tensor.
 * Synchronises `stream`.  OPUS_EBADARG when a weight is not finite (the outputs are then not to be used).  Added within ABI 10. */
int opus_quantize_fp8(const void *d_src, int64_t N, int64_t K, void *d_q8, void *d_e8, void *d_dq, void *stream);

/* MXFP4 decoder weights (OCP MX v1.0: e2m1 elements, one e8m0 scale per 32 consecutive k of a row; 4.25 bits per weight).  Like
 * FP8 a decode-throughput option and a different model, not a capacity option: the operand-type tensors stay bound.  Quantises
 * one decoder-layer weight after all load-time fusion and before tiling: row-major W[N,K] in the operand type (N % 16 == 0,
 * K % 64 == 0) ->
 *   d_s4  N K / 32 bytes  scale byte e + 127 of block (n, kb = k / 32), e = floor(log2(absmax_block)) - 2 (never below -120; 0 for
 *                         an all-zero block), in scale panels: block (p = n / 16, c = k / 64) is the 32 B at ((p K / 64) + c) 32,
 *                         row n = 16 p + li owns bytes 2 li (kb even) and 2 li + 1 (kb odd)
 *   d_q4  N K / 2 bytes   e2m1 codes, magnitude RNE(min(|W| 2^-e, 6)) over {0, 0.5, 1, 1.5, 2, 3, 4, 6} (ties to the even code),
 *                         sign in bit 3, two per byte with the lower k in the low nibble, in code panels: block (p, c) is the 512 B
 *                         at ((p K / 64) + c) 512; lane g 16 + li owns 8 bytes, bytes 0..3 = k 64 c + 8 g + 0..7, bytes 4..7 =
 *                         k 64 c + 32 + 8 g + 0..7.  A code whose value q 2^e would be subnormal in the operand type is +0, and so
 *                         is a negative zero
 *   d_dq  (optional)      q 2^e in the operand type, row-major [N,K], exact; may be d_src (in place)
 * Bind q4 / s4 as "dec.{l}.{wqkv,wo,wgu,wd}.q4" (OPUS_F4E2M1X2 [N,K/2]) / ".s4" (OPUS_E8M0 [N,K/32]) beside the panel-tiled dq
 * bound under the usual name (Llama / Qwen2 layers; both tensors of a projection or neither, and not beside its FP8 form): the
 * decode step's GEMMs that have an MXFP4 form (the kernels that have an FP8 form) then stream 0.27 of the bytes of the same
 * numbers; every other launch reads the operand-type tensor.  Synchronises `stream`.  OPUS_EBADARG when a weight is not finite
 * (the outputs are then not to be used).  Added within ABI 10. */
int opus_quantize_mxfp4(const void *d_src, int64_t N, int64_t K, void *d_q4, void *d_s4, void *d_dq, void *stream);

/* Rows E1-E4: ProteinSeqEmbeddingExtractor.get_protein_seq_embeddings (cstp_v3/modelling.py:37-57):
 * tokens int32 [B,T] (<cls> seq <eos>, pad = 1), lens int32 [B] (incl. <cls>,<eos>) ->
 * pooled fp32 [B, enc_dim] = mean over residues of representations[enc_layers]. */
int opus_esm2_encode(opus_ctx *ctx, const int32_t *d_tokens, const int32_t *d_lens, int32_t B, int32_t T,
                     float *d_pooled, void *stream);
/* The same rows on a TOKEN-PACKED batch (no padding: the reference pads to the longest protein of the batch,
 * cstp_v3/modelling.py:44-46, and multiplies the padding): d_tokens int32 [cu[B]] = the proteins' tokens (<cls> seq <eos>) back
 * to back, h_cu (HOST) int32 [B + 1] their row offsets (cu[0] = 0; 2 <= cu[b+1] - cu[b] <= max_enc_tokens;
 * cu[B] <= max_batch * max_enc_tokens) -> pooled fp32 [B, enc_dim], the same values as opus_esm2_encode gives each protein
 * (different GEMM tile boundaries: equal to the tolerance of DESIGN.md section 3, not bitwise).  Mixed lengths need no buckets.
 * opus_esm2_last_hidden(ctx, out, 1, cu[B]) then returns the packed [cu[B], enc_dim] representations of the RESIDUE rows; the
 * <cls> / <eos> rows, which the mean-pool drops, are not computed by the last layer (knob "enc_full_last_layer" = 1: they are). */
int opus_esm2_encode_packed(opus_ctx *ctx, const int32_t *d_tokens, const int32_t *h_cu, int32_t B, float *d_pooled, void *stream);
/* Debug/parity tap: copy of representations[enc_layers] fp32 [B,T,enc_dim] of the last encode. */
int opus_esm2_last_hidden(opus_ctx *ctx, float *d_out, int32_t B, int32_t T, void *stream);

/* Rows P1+P2: encode_projector_embedding + switch_projector_embedding (opus_arch.py:115-131,
 * modelling.py:396-400, protein_mlp/builder.py:11-25): pooled fp32 [B,enc_dim] ->
 * fp16 [B, n_prot_tokens, dec_dim].  d_proj_out (optional, may be NULL) receives the P1 output
 * fp16 [B, proj_dim].  B is NOT limited by max_batch: the batched stage of the two-stage pipeline (SURVEY 8f N3,
 * opus_arch.py:151-161 + scripts/generate_esm_embedding.py) projects whole dataset shards at M >= 512, in chunks of
 * max(max_batch, 4096) rows.  has_protein_projector = 0 is the identity module of opus_arch.py:70-80: P1 is a cast. */
int opus_projector_forward(opus_ctx *ctx, const float *d_pooled, int32_t B, void *d_out, void *d_proj_out,
                           void *stream);
/* Row P1 alone: encode_projector_embedding (opus_arch.py:115-121): fp32 [B,enc_dim] -> fp16 [B,proj_dim]. */
int opus_protein_projector(opus_ctx *ctx, const float *d_pooled, int32_t B, void *d_out, void *stream);
/* Row P2 alone: switch_projector_embedding (opus_arch.py:122-131): fp16 [B,switch_in] -> fp16 [B,n,H]. */
int opus_switch_projector(opus_ctx *ctx, const void *d_in, int32_t B, void *d_out, void *stream);

/* Rows S1-S3: the splice of prepare_inputs_labels_for_multimodal (opus_arch.py:166-270).
 * ids int64 [B,T_text] (-200 = <seq>), mask u8 [B,T_text] (NULL = all ones), prot fp16
 * [n_prot, n_prot_tokens, dec_dim] consumed in order (a row without placeholder consumes one).
 * Outputs sized for max_prompt: embeds fp16 [B,T_out,H] (zeros in pad slots), mask u8 [B,T_out],
 * pos int32 [B,T_out].  T_out is a HOST int: the call synchronises `stream` once to return it.
 * max_length > 0 truncates rows (config.tokenizer_model_max_length, :234-237).
 * Errors: OPUS_ESHAPE when fewer protein blocks are supplied than the rows consume, or T_out
 * exceeds max_prompt. */
int opus_splice_pad(opus_ctx *ctx, const int64_t *d_ids, const uint8_t *d_mask, int32_t B, int32_t T_text,
                    const void *d_prot, int32_t n_prot, int32_t inference_mode, int32_t max_length,
                    void *d_embeds, uint8_t *d_mask_out, int32_t *d_pos_out, int32_t *T_out, void *stream);

/* Rows D1,D2,D4: LlamaForCausalLM prefill as called by generate (language_model/opus_llama.py:127-132):
 * embeds fp16 [B,T,H], mask u8 [B,T] (left-padded rows) -> logits of the LAST position fp32 [B,V];
 * fills the context's KV cache and resets its step counter. */
int opus_llama_prefill(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                       float *d_last_logits, void *stream);
/* opus_llama_prefill on B prompts that leaves B nret decoder rows (generate(num_return_sequences=nret): the prompt is prefilled
 * once, on B rows; B nret <= max_batch, else OPUS_ESHAPE; nret < 1: OPUS_EBADARG).  Afterwards the context is as after a prefill
 * of every prompt repeated nret times (transformers' _expand_inputs_for_generation, row b nret + j = prompt b): the KV cache rows
 * b nret + j hold prompt b's keys and values in every layer (the cache append stores them nret times from registers), the
 * first-slot table and the last-position logits are replicated, and opus_llama_decode_step, opus_last_logits and opus_kv_reorder
 * work on B nret rows.  The prefill's arithmetic is that of the plain B-row call: the logits of rows b nret + j are bit-identical
 * to its row b.  d_last_logits (optional) fp32 [B nret, V].  nret == 1: exactly opus_llama_prefill. */
int opus_llama_prefill_fanout(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t nret,
                              float *d_last_logits, void *stream);
/* Row D3: one decode step for the B rows of the last prefill: tok int32 [B] -> logits fp32 [B,V]. */
int opus_llama_decode_step(opus_ctx *ctx, const int32_t *d_tok, float *d_logits, void *stream);

/* Teacher-forced scoring (the reference's forward(labels=...), opus_llama.py:41-92): the prefill's layers run on EVERY position
 * (embeds fp16 [B,T,H], mask u8 [B,T]: right-padded, unpadded or left-padded rows, positions t - first valid slot), then for the
 * R flat positions d_rows[r] = b T + t (int32, device) the final norm + lm_head give operand-dtype logits and
 * d_logprob[r] = log_softmax(logits)[d_targets[r]] (fp32; a target < 0 gives 0).  d_logits [R, V] (operand dtype, row r = position
 * d_rows[r]) or NULL: loss-only, the logits live chunk by chunk in d_scratch (at most 128 MiB of them per chunk).  d_scratch
 * (device, scratch_bytes) holds the gathered rows (+ the chunk's logits): opus_llama_forward_scratch_bytes says what it takes
 * (less: smaller chunks).  Overwrites the context's KV cache and leaves it without a prefill: opus_llama_decode_step then fails
 * with OPUS_ESTATE until the next prefill / generate.  opus_workspace_bytes is unchanged by it. */
int opus_llama_forward(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, const int32_t *d_rows,
                       int32_t R, const int32_t *d_targets, float *d_logprob, void *d_logits, void *d_scratch,
                       int64_t scratch_bytes, void *stream);
/* Scratch bytes opus_llama_forward wants for R scored rows (with_logits: d_logits is given); -1 on a bad config. */
int64_t opus_llama_forward_scratch_bytes(const opus_config *cfg, int32_t R, int32_t with_logits);
/* Shared-prefix scoring.  opus_llama_prefix is opus_llama_prefill (same cache, step counter and decode state afterwards:
 * opus_llama_decode_step continues it) that also copies the final residual rows of every row's LAST position, fp32 [B, H], into
 * d_last_rows and returns the cache epoch in *epoch.  The last slot of every row must be a real token (left-padded or unpadded
 * rows).  The prefix stays valid until the next call on this context that prefills or permutes the cache (opus_llama_prefill /
 * _prefix / _forward, opus_generate_*, opus_kv_reorder, the debug attention entries); decode steps keep it. */
int opus_llama_prefix(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, float *d_last_logits,
                      float *d_last_rows, int64_t *epoch, void *stream);
/* Scores R continuation rows behind the prefix of `epoch` (OPUS_ESTATE when it is stale or from another context).  d_embeds
 * operand dtype [R, n, H]: row r's token embeddings, right-padded to n positions (1 <= n <= max_prompt, else OPUS_ESHAPE);
 * h_lens [R] (host): real tokens per row (0 .. n); h_src [R] (host): prefix row of every row (0 .. P - 1, repeats and any order);
 * d_last_rows fp32 [P, H]: what opus_llama_prefix returned, P = its B.  Token j of row r sits at position Tp - kstart + j of its
 * prefix row (at most max_prompt + max_new_tokens positions in all, else OPUS_ESHAPE).  Output, compact over the real tokens in
 * row-major order (row 0's lens[0] tokens, then row 1's ...): d_logprob[k] = log p(d_targets[k] | prefix, earlier tokens of the
 * row) in fp32; token 0 of a row is scored from the prefix's last position.  Reads the KV cache and writes neither it nor the
 * decode state: the same prefix can be scored any number of times and decoded afterwards.  Rows run in passes of as many as the
 * prefill's activation buffers hold positions (max_batch x max_prompt); d_scratch (device) holds
 * opus_llama_score_scratch_bytes(cfg, R, n) bytes.  Phase "score"; the attention kernel is timed as class "attn_prefill". */
int opus_llama_score_continuations(opus_ctx *ctx, const void *d_embeds, int32_t R, int32_t n, const int32_t *h_lens,
                                   const int32_t *h_src, const float *d_last_rows, int32_t P, int64_t epoch,
                                   const int32_t *d_targets, float *d_logprob, void *d_scratch, int64_t scratch_bytes, void *stream);
/* Scratch bytes opus_llama_score_continuations needs for R rows of n positions; -1 on a bad config or R < 1, n < 1, n > max_prompt. */
int64_t opus_llama_score_scratch_bytes(const opus_config *cfg, int32_t R, int32_t n);
/* attn_prefix_kernel alone, on layer 0 of this context's KV cache: d_k_hist / d_v_hist fp16 [P, kv, Tp, hd] (keys rotated) go to
 * slots 0 .. Tp - 1, d_kstart int32 [P] (device) is the first visible slot of each prefix row; d_qkv [R n, (heads + 2 kv) hd]: the
 * continuation rows' q | k | v, q and k rotated; h_src [R] (host) their prefix rows.  Query t of row r attends to slots
 * kstart[p] .. Tp - 1 of p = h_src[r] and to positions 0 .. t of its own row.  d_out [R n, heads hd].  Leaves the context
 * without a prefill. */
int opus_debug_attn_prefix(opus_ctx *ctx, const void *d_qkv, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                           int32_t P, int32_t Tp, int32_t R, int32_t n, const int32_t *h_src, void *d_out, void *stream);
/* Trie scoring: exact log-probabilities of every member of a token trie behind the prefix of `epoch`, one tree pass (the planner
 * is opus-pllm_amd/constraint.py plan_trie_score; OpusLlamaForCausalLM.score_trie drives it).  One call = one pass of `rows` trie
 * nodes (0 <= rows <= opus_llama_dec_rows_cap), each ONE new position: d_embeds operand dtype [rows, H]; host tables h_src (prefix
 * row), h_par (parent row in this pass, -1 for a child of the root; otherwise an EARLIER row of the same prefix row one level up)
 * and h_depth (1 .. opus_llama_tree_max_depth(), else OPUS_ESHAPE).  A row at depth d sits at position Tp - kstart + d - 1 of its
 * prefix row (at most max_prompt + max_new_tokens positions in all, else OPUS_ESHAPE) and attends to the prefix row's cache slots,
 * its ancestors and itself (attn_prefix_kernel, tree form).  Scoring: h_score_src [n_score] lists the rows whose logits are needed - a row
 * of the pass, or -(p) - 1 for the last position of prefix row p (d_last_rows fp32 [P, H] of opus_llama_prefix); the lm_head runs
 * once per entry.  Edge e (h_edge_row ascending indices into that list, h_edge_tok, h_edge_slot) writes
 * d_node_lp[slot] = log_softmax(logits(row))[tok]; stop entry k (h_stop_row ascending, h_stop_set, h_stop_slot) writes
 * d_stop_lp[slot] = log sum over the ids h_stop_ids[h_stop_off[set] .. h_stop_off[set + 1]) of softmax(logits(row))[id].  Slots lie
 * in [0, n_slots); a slot no entry names is left as it was.  Every table is checked on the host (OPUS_EBADARG).  Reads the KV
 * cache and writes neither it nor the decode state (OPUS_ESTATE on a stale or foreign epoch); fixed summation orders, no float
 * atomics: the same inputs give bitwise the same outputs.  d_scratch holds opus_llama_score_tree_scratch_bytes(...) bytes; the
 * context's workspace does not grow.  Returns after the stream has finished.  Phase "score". */
int opus_llama_score_tree(opus_ctx *ctx, const void *d_embeds, int32_t rows, const int32_t *h_src, const int32_t *h_par,
                          const int32_t *h_depth, int32_t n_score, const int32_t *h_score_src, int32_t n_edges,
                          const int32_t *h_edge_row, const int32_t *h_edge_tok, const int32_t *h_edge_slot, int32_t n_stops,
                          const int32_t *h_stop_row, const int32_t *h_stop_set, const int32_t *h_stop_slot, int32_t n_stop_ids,
                          const int32_t *h_stop_ids, int32_t n_stop_sets, const int32_t *h_stop_off, const float *d_last_rows,
                          int32_t P, int64_t epoch, float *d_node_lp, float *d_stop_lp, int64_t n_slots, void *d_scratch,
                          int64_t scratch_bytes, void *stream);
/* Scratch bytes of one opus_llama_score_tree pass; -1 on a bad config, a negative count or rows above opus_llama_dec_rows_cap. */
int64_t opus_llama_score_tree_scratch_bytes(const opus_config *cfg, int32_t rows, int32_t n_score, int32_t n_edges, int32_t n_stops,
                                            int32_t n_stop_ids, int32_t n_stop_sets);
/* Positions the decoder's activation buffers hold: the rows of one pass of opus_llama_score_tree / _score_continuations
 * (max(max_batch x max_prompt, max_batch rounded up to 16)); -1 on a bad config. */
int64_t opus_llama_dec_rows_cap(const opus_config *cfg);
/* Deepest trie node opus_llama_score_tree takes (64). */
int32_t opus_llama_tree_max_depth(void);
/* member_lp[p, m] = the sum of d_node_lp[p, v] over the path of node d_member_node[d_trie[p], m], added in fp32 from the root to
 * the leaf (-inf where that node is < 0).  d_par / d_depth int32 [tries, ld_nodes] (node 0 = the root), d_node_lp fp32
 * [P, ld_nodes], d_member_node int32 [tries, M], d_trie int32 [P], d_member_lp fp32 [P, M]; all device. */
int opus_trie_path_sums(opus_ctx *ctx, const float *d_node_lp, const int32_t *d_trie, const int32_t *d_par, const int32_t *d_depth,
                        const int32_t *d_member_node, int32_t P, int32_t M, int32_t ld_nodes, float *d_member_lp, void *stream);
/* attn_prefix_kernel's tree form alone, on layer 0 of this context's KV cache: the arguments of opus_debug_attn_prefix with one position per row
 * (d_qkv [R, (heads + 2 kv) hd]) and the host tables h_par / h_depth [R] of opus_llama_score_tree.  Row r attends to slots
 * kstart[p] .. Tp - 1 of p = h_src[r], to its ancestors and to itself.  d_out [R, heads hd].  Leaves the context without a prefill. */
int opus_debug_attn_tree(opus_ctx *ctx, const void *d_qkv, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                         int32_t P, int32_t Tp, int32_t R, const int32_t *h_src, const int32_t *h_par, const int32_t *h_depth,
                         void *d_out, void *stream);
/* Trie search (OpusLlamaForCausalLM.search_trie): beam search for the best members of a token trie behind a cached prefix.  The
 * decoder runs P x K rows (row p K + k = beam k of prompt p) through opus_llama_prefill_behind / opus_llama_decode_step; between
 * two passes opus_trie_search_level expands every prompt's beams on the device (trie_beam_expand_kernel, one workgroup per
 * prompt), its `parent` array is what opus_kv_reorder takes and its `tok` array what the next step takes.
 *
 * opus_set_trie_search uploads the table (host arrays, copied to a device allocation the context owns; returns after the stream
 * has finished): the tries' children in CSR form - state s owns edges edge_off[s] .. edge_off[s + 1), ids ascending and inside the
 * vocabulary, edge_next the child states; member[s] >= 0: the member index of a state that completes a member (-1 otherwise);
 * stop_set[s] in [0, n_sets): the id set of the state's trie, ids stop_ids[stop_off[set] .. stop_off[set + 1]) (at least one id per
 * set).  State 0 is the dead state: no edges, no member.  Every array is checked (OPUS_EBADARG); n_edges < 2^27. */
int opus_set_trie_search(opus_ctx *ctx, int32_t n_states, const int32_t *edge_off, const int32_t *edge_tok, const int32_t *edge_next,
                         int32_t n_edges, const int32_t *member, const int32_t *stop_set, int32_t n_sets, const int32_t *stop_off,
                         const int32_t *stop_ids, void *stream);
/* One level's device arrays, P prompts x K beams (1 <= top <= K <= 16).  Beam k of prompt p stands in state state[p K + k] with
 * the running score score[p K + k] (-inf or state 0: dead).  The call replaces both by the K best continuations (score descending,
 * ties to the lower (beam, id); dead: state 0, -inf), writes their ids to tok (dead: a valid id), the ROW p K + k' each continues to
 * parent (dead: its own row) and, optionally, the edge's log-prob to edge_lp and each old beam's stop term to beam_stop.  The
 * pool (pool_member -1 / pool_lp -inf / pool_stop -inf = empty) keeps the best `top` members by pool_lp + pool_stop, ties to the
 * lower member index.  flags [P, 3]: {live, exhaustive, some beam changes its row}; set {1, 1, 0} before the first level.  A
 * prompt whose best beam is strictly below its top-th pool entry, or that has no beam left, stops: live = 0, all beams dead.
 * d_words [2] receives {prompts still live, prompts whose beams change rows}; d_lse [rows] is scratch for the rows' log-sum-exp. */
typedef struct opus_trie_search_io {
    int32_t P, K, top, include_stop;
    int32_t *d_state;
    float *d_score;
    int32_t *d_tok, *d_parent;
    int32_t *d_pool_member;
    float *d_pool_lp, *d_pool_stop;
    int32_t *d_flags;
    int32_t *d_words;
    float *d_lse;
    float *d_edge_lp, *d_beam_stop;   /* optional (NULL: off) */
} opus_trie_search_io;
/* The first level's logits: final norm + lm_head of d_last_rows fp32 [P, H] (opus_llama_prefix's last rows) into the context's
 * logits, one row per prompt.  The context is left without a prefill (opus_llama_prefill_behind follows). */
int opus_trie_search_begin(opus_ctx *ctx, const float *d_last_rows, int32_t P, void *stream);
/* One level on the context's logits: first != 0: the P rows opus_trie_search_begin left (only beam 0 of a prompt is read);
 * otherwise the P K rows of the last prefill / decode step (OPUS_ESHAPE when that had another row count).  Needs
 * opus_set_trie_search (OPUS_ESTATE).  Reads the logits, never writes them; fixed orders, bitwise repeatable.  Phase "decode". */
int opus_trie_search_level(opus_ctx *ctx, const opus_trie_search_io *io, int32_t first, void *stream);
/* Diagnostic: the same launch on caller logits fp32 [rows, V] (rows = P when first != 0, else P K; P K <= max_batch); the table's ids
 * must lie below V.  d_lse of `io` receives the rows' log-sum-exp as the kernel used it. */
int opus_debug_trie_beam_expand(opus_ctx *ctx, const float *d_logits, int32_t V, const opus_trie_search_io *io, int32_t first,
                                void *stream);
/* ESM-2 contact maps (EsmContactPredictionHead / fair-esm return_contacts=True) beside the per-residue states, on the token-packed
 * encoder: the same arguments and pooled output as opus_esm2_encode_packed, then d_contacts fp32 receives protein b's [n_b, n_b]
 * map (n_b = cu[b + 1] - cu[b] - 2 residues, row-major) at element offset sum_{b' < b} n_{b'}^2.  Needs the optional weights
 * "enc.contact.weight" fp32 [enc_layers * enc_heads] (channel l * enc_heads + h) and "enc.contact.bias" fp32 [1] (OPUS_ESTATE
 * names the missing one).  d_scratch (256-byte aligned) holds opus_esm2_contacts_scratch_bytes(cfg, h_cu, B) bytes: the context's
 * workspace does not grow.  opus_esm2_last_hidden afterwards returns every residue row.  Phase "encode", kernel class "contact". */
int opus_esm2_contacts_packed(opus_ctx *ctx, const int32_t *d_tokens, const int32_t *h_cu, int32_t B, float *d_pooled, float *d_contacts,
                              void *d_scratch, int64_t scratch_bytes, void *stream);
/* Scratch bytes of opus_esm2_contacts_packed for these proteins (about 4 sum n^2 + 4 sum n * layers * heads); -1 on bad arguments. */
int64_t opus_esm2_contacts_scratch_bytes(const opus_config *cfg, const int32_t *h_cu, int32_t B);
/* ESM-2 masked-LM head (fair-esm RobertaLMHead / transformers EsmLMHead) on the final states the last opus_esm2_encode* /
 * opus_esm2_contacts_packed call left in the context: d_out fp32 [R, enc_vocab] = LN(gelu(h Wd^T + bd)) We^T + b for the R rows
 * d_rows (device int32) names on that call's token axis (packed: 0 .. cu[B] - 1; padded: b T + t); the list may be unsorted and
 * may repeat, an index outside the axis gives a NaN row; NULL means rows 0 .. R - 1.  log_softmax != 0: the log-softmax over the
 * enc_vocab columns instead of the logits.  After a packed call the <cls> / <eos> rows hold no state (see opus_esm2_encode_packed).
 * Needs the optional weights "enc.lm.dense.weight" (operand type, panel-tiled [enc_dim, enc_dim]), "enc.lm.dense.bias",
 * "enc.lm.ln.weight", "enc.lm.ln.bias" fp32 [enc_dim], "enc.lm.bias" fp32 [enc_vocab] and, when the output projection is not tied
 * to the token embedding, "enc.lm.weight" (operand type, row-major [enc_vocab, enc_dim]).  Errors: OPUS_ESTATE when the context
 * holds no complete encoder result (none yet, one that failed, or opus_debug_esm2_lm_head since); OPUS_EBADARG when the head is
 * not bound (the message names the tensors); OPUS_ESHAPE for R outside 1 .. max_batch * max_enc_tokens (without a list: the
 * call's rows).  Up to 128 rows the dense step has one launch shape: a row's result does not depend on the other rows of the
 * call.  Touches neither the KV cache nor the decode state.  Phase "encode", kernel class "mlm" (+ the dense step's GEMM class). */
int opus_esm2_lm_head(opus_ctx *ctx, const int32_t *d_rows, int32_t R, int32_t log_softmax, float *d_out, void *stream);
/* The same two steps on caller-supplied fp32 states d_hidden [R, enc_dim] (kernel tests).  The states are staged where the
 * encoder leaves its own, so the context holds no encoder result afterwards. */
int opus_debug_esm2_lm_head(opus_ctx *ctx, const float *d_hidden, int32_t R, int32_t log_softmax, float *d_out, void *stream);
/* Diagnostic: one layer's contact accumulation alone.  d_q / d_k: operand-dtype rows of stride ld elements, head h at column
 * h * head_dim (q already scaled, both rotated), token-packed proteins h_cu[B + 1] (host, at least 2 tokens each).  Over the
 * interior positions (tokens 1 .. n_b) of P_h = softmax over all of the protein's keys of q k^T: d_A [sum n_b^2] =
 * sum_h d_w[h] P_h (packed as in opus_esm2_contacts_packed), d_rows / d_cols [sum n_b][heads] the interior row / column sums of
 * P_h (protein b's rows from cu[b] - 2 b).  d_scratch: 256 + 4 (B + 1) + 4 heads sum_b ceil(n_b / 64) n_b bytes or more. */
int opus_debug_contacts(opus_ctx *ctx, const void *d_q, const void *d_k, int64_t ld, const int32_t *h_cu, int32_t B, int32_t heads,
                        int32_t head_dim, const float *d_w, float *d_A, float *d_rows, float *d_cols, void *d_scratch,
                        int64_t scratch_bytes, void *stream);
/* Diagnostic: the NLL kernel alone.  Per row of operand-dtype logits [R, V] (row-major): d_lse[r] = logsumexp (fp32, d_lse may
 * be NULL) and d_logprob[r] = l[y] - lse with y = d_targets[r] (y < 0: 0; y >= V: NaN). */
int opus_debug_xent(opus_ctx *ctx, const void *d_logits, int32_t R, int32_t V, const int32_t *d_targets, float *d_logprob,
                    float *d_lse, void *stream);

/* Rows G1 (+D1-D4): greedy search of GenerationMixin as driven by opus_llama.py:95-132.
 * next = argmax(last logits); finished rows emit pad_id; a row finishes on any of eos_ids (host
 * array, may be empty); stops when all rows are finished or after max_new steps.
 * out ids int32 [B,max_new] (device; unused tail = pad_id); n_out (HOST) = steps produced, the
 * second dimension HF would return.  Synchronises `stream` (it returns a host scalar). */
int opus_generate_greedy(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                         int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id,
                         int32_t *d_out_ids, int32_t *n_out, void *stream);

/* Row N2, "### early-stop as an opt-in" (the reference decodes to max_new_tokens and cuts the text at the first "###"
 * afterwards, eval/run_opus_ddp.py:19-27): with the token ids of "###" set here (HOST array, at most 8; n = 0 clears), a row
 * is finished once its new ids end with that sequence - later positions hold pad_id, as after an EOS - so the text after the
 * cut is unchanged and a batch can stop early.  Applies to opus_generate_greedy / opus_generate_sample of this context. */
int opus_set_stop_sequence(opus_ctx *ctx, const int32_t *ids, int32_t n);

/* Row N1 (sampling head, the reference's default decode mode: run_opus_ddp.py:126-128,156-157 temperature 0.1,
 * top_p 0.7): same loop with next = multinomial(softmax(top_p_filter(logits / temperature))) per transformers'
 * TemperatureLogitsWarper + TopPLogitsWarper; draws come from a counter-based generator keyed by
 * (seed, row, step), so a given seed reproduces its tokens.  Parity with the reference is distributional. */
int opus_generate_sample(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T,
                         int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature,
                         float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out, void *stream);
/* Diagnostic: one draw per row of fp32 logits [B, dec_vocab] (synchronises the stream). */
int opus_debug_sample(opus_ctx *ctx, const float *d_logits, int32_t B, float temperature, float top_p, uint64_t seed,
                      int32_t step, int32_t *d_tokens, void *stream);

/* generate(return_dict_in_generate=True, output_*=True): opus_generate_greedy (temperature == 0; top_p and seed unused) or
 * opus_generate_sample (temperature > 0) that also returns, per generated step, what the caller asks for (NULL = off; caller
 * memory, fp32):
 *   d_token_logprobs [B, max_new]: log p(chosen token) under the model's distribution (temperature 1, no filters); 0 for a row
 *     that finished before the step (its EOS / last stop-sequence token still counts).  The log-sum-exp is fused into the
 *     arg-max pass over the logits.
 *   d_scores [max_new, B, dec_vocab]: HF's processed scores - greedy: the logits; sampling: logits / temperature where the draw's
 *     top-k / top-p filters kept the token (the draw's own keep test), -inf elsewhere.
 *   d_logits [max_new, B, dec_vocab]: the raw logits.
 * Steps at and past *n_out hold nothing defined.  The output addresses reach the captured decode step through a small device
 * descriptor written before the loop: each call may pass fresh buffers without a new graph; which outputs are on is part of the
 * graph's identity.  All three NULL: exactly opus_generate_greedy / _sample (same launches, same graph). */
int opus_generate_scored(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                         const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature, float top_p, uint64_t seed,
                         int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs, float *d_scores, float *d_logits,
                         void *stream);
/* opus_generate_scored with nret decoder rows per prompt: embeds / mask carry B prompts, prefilled once (opus_llama_prefill_fanout);
 * the loop, d_out_ids [B nret, max_new] and the outputs ([B nret, max_new], [max_new, B nret, V]) are those of a B nret-row batch,
 * decoder row r = b nret + j being the j-th sample of prompt b with its draws keyed by (seed, r, step).  EOS ids, the stop
 * sequence, the logits processors and the token constraint act per decoder row; a constraint with B start states gives row r the
 * start state r / nret.  The captured step is that of a B nret-row batch (no graph of its own).  nret == 1: exactly
 * opus_generate_scored. */
int opus_generate_scored_fanout(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t nret,
                                int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature,
                                float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs,
                                float *d_scores, float *d_logits, void *stream);

/* opus_generate_scored with classifier-free guidance (generate(guidance_scale=g); transformers'
 * UnbatchedClassifierFreeGuidanceLogitsProcessor) on paired rows.  d_embeds [2 P, T, dec_dim] / d_mask [2 P, T]: rows [0, P) the
 * conditional prompts, rows [P, 2 P) their negative prompts, all left-padded to one length T.  One 2 P-row prefill; every step
 * decodes 2 P rows, and its head works on the first P:
 *   1. the raw outputs of the conditional rows are taken (d_logits, the log-sum-exp behind d_token_logprobs);
 *   2. scores[b] = g ((l_c - lse_c) - (l_u - lse_u)) + (l_u - lse_u), l_u = row P + b, overwrites row b in fp32;
 *   3. the logits processors, the token constraint, then temperature / top-k / top-p;
 *   4. the arg-max or the draw (keyed by (seed, b, step)) on the P rows;
 *   5. row P + b is fed the token chosen for row b (pad_id once row b has finished).
 * EOS ids, the stop sequence, processor histories and constraint states (one start state, or P) exist for the P rows only.
 * d_out_ids [P, max_new], d_token_logprobs [P, max_new] (raw, conditional), d_scores [max_new, P, V] (guided and processed),
 * d_logits [max_new, P, V] (raw, conditional).  guidance_scale reaches the step through a device word: the captured step is that of
 * a 2 P-row batch with "guided" in its identity, shared by every scale.  A guided call of P prompts costs about a plain call of
 * 2 P rows.  OPUS_EBADARG: guidance_scale not finite; OPUS_ESHAPE: 2 P > max_batch, T > max_prompt.  Added within ABI 10 (a new
 * symbol only). */
int opus_generate_scored_guided(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t P, int32_t T, float guidance_scale,
                                int32_t max_new, const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature,
                                float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out, float *d_token_logprobs,
                                float *d_scores, float *d_logits, void *stream);

/* Detached prefixes (added within ABI 10).  A snapshot is the K and V of a prefill's rows copied out of the context's cache into
 * memory the caller owns: d_k / d_v operand dtype [dec_layers][P][dec_kv_heads][Tp][dec_head_dim] (slot 0 first), d_kstart int32 [P]
 * (device) the first real slot of every row, h_kstart the same on the host.  It never goes stale, can be used any number of times
 * and from every context of the same configuration and weights.  K is stored rotated by slot - kstart, so a row's slots can be
 * placed at other slots unchanged as long as kstart moves with them. */
typedef struct opus_prefix_snap {
    const void *d_k, *d_v;
    const int32_t *d_kstart, *h_kstart;
    int32_t P, Tp;
} opus_prefix_snap;
/* Bytes of d_k plus d_v (each half of it) of a snapshot of P rows x Tp slots: 2 * dec_layers * P * dec_kv_heads * Tp * dec_head_dim
 * * 2; -1 on a bad config or P outside 1 .. max_batch, Tp outside 1 .. max_prompt + max_new_tokens. */
int64_t opus_llama_prefix_bytes(const opus_config *cfg, int32_t P, int32_t Tp);
/* Strided copy-out of the live cache: rows 0 .. R - 1, slots 0 .. T - 1 of every layer -> d_k / d_v [dec_layers][R][dec_kv_heads][T]
 * [dec_head_dim], and (d_kstart not NULL) the rows' kstart -> d_kstart [R].  `epoch`: what opus_llama_prefix /
 * opus_llama_prefill_behind returned; OPUS_ESTATE when the cache has been prefilled or permuted since.  Decode steps keep the epoch:
 * T may reach past the prompt to read the slots they appended.  Changes nothing in the context. */
int opus_llama_prefix_export(opus_ctx *ctx, int64_t epoch, int32_t R, int32_t T, void *d_k, void *d_v, int32_t *d_kstart, void *stream);
/* Prefill behind a prefix: the snapshot + R suffix rows -> the context state of opus_llama_prefill on the concatenated prompts,
 * without running the prefix again.  d_embeds operand dtype [R, n, H]: the suffix embeddings, RIGHT-padded to n positions; h_lens
 * [R] (host) 1 <= n_r <= n; h_src [R] (host) the snapshot row of every decode row (any order, repeats, rows may go unused).
 * Afterwards (T' = Tp + n, p = h_src[r], d_r = n - n_r): kstart'[r] = kstart[p] + d_r, the prefix of row r sits at slots
 * kstart'[r] .. kstart'[r] + Tp - kstart[p] - 1 (kv_place_kernel: one launch, all layers, bits unchanged), suffix position t at slot
 * Tp + d_r + t, every row ends at T' - 1, the last-position logits fp32 [R, V] are left for the decode loop (and copied to
 * d_last_logits when not NULL), the step counter is 0, *epoch (when not NULL) the new cache epoch.  Slots below kstart'[r] and rows
 * >= R are not written.  The suffix pass is the prefill's layer loop on R n rows with attn_prefix_kernel reading the snapshot; every
 * position runs through the last layer (no last-layer shortcut).  OPUS_ESHAPE unless R <= max_batch, Tp + n <= max_prompt,
 * R n <= max_batch max_prompt and 1 <= n_r <= n; OPUS_EBADARG for a row of h_src outside the snapshot. */
int opus_llama_prefill_behind(opus_ctx *ctx, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                              const int32_t *h_lens, const int32_t *h_src, float *d_last_logits, int64_t *epoch, void *stream);
/* opus_llama_prefill_behind that also leaves a LIVE prefix on the context, as opus_llama_prefix does for a plain prefill: the final
 * residual rows of the R rows' last positions -> d_last_rows fp32 [R, H] (required), the rows' kstart' is kept on the host, *epoch
 * (required) is the new cache epoch.  Afterwards opus_llama_score_continuations / opus_llama_score_tree / opus_llama_prefix_export
 * take (P = R, *epoch) with Tp + n slots per row.  Everything else - arguments, checks, launches, the decode state - is
 * opus_llama_prefill_behind's.  Added within ABI 10 (a new symbol only). */
int opus_llama_prefix_behind(opus_ctx *ctx, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                             const int32_t *h_lens, const int32_t *h_src, float *d_last_logits, float *d_last_rows, int64_t *epoch,
                             void *stream);
/* Ragged copy-out of the cache a decode loop leaves behind (kv_export_rows_kernel: K and V of all layers in one launch, bits
 * unchanged).  T0 = the slot count of the context's last prefill (plain, fanned out or behind a prefix), kstart = the context's own.
 * Row r's window is slots kstart[r] .. T0 + h_keep[r] - 1 (h_keep HOST [R]: how many of the slots the decode steps appended belong
 * to the row), L_r = T0 - kstart[r] + h_keep[r] of them.  It is written to d_k / d_v [dec_layers][R][dec_kv_heads][Tp_out]
 * [dec_head_dim] at slots Tp_out - L_r .. Tp_out - 1 - every row ends at the last slot, as opus_llama_prefill_behind expects of a
 * snapshot - with zeros in every slot below, and d_kstart_out[r] = Tp_out - L_r (device int32 [R], required).  The whole snapshot is
 * written: two exports of one state are bit-identical.  OPUS_ESTATE when the context holds no prefill (or a continuous session is
 * open); OPUS_ESHAPE when R is not the row count of the last step, an h_keep[r] is negative or above the number of decode steps
 * that ran since the prefill, Tp_out < max L_r or Tp_out > max_prompt + max_new_tokens (opus_llama_prefix_bytes' range).  Reads the
 * step word and kstart back (synchronises the stream once); changes nothing in the context, the epoch included.  Added within
 * ABI 10 (a new symbol only). */
int opus_llama_prefix_export_rows(opus_ctx *ctx, int32_t R, const int32_t *h_keep, int32_t Tp_out, void *d_k, void *d_v,
                                  int32_t *d_kstart_out, void *stream);
/* opus_generate_scored with its prefill replaced by opus_llama_prefill_behind (greedy: temperature == 0; outputs optional, all NULL:
 * the plain loop).  Everything behind the prefill is that of an R-row batch: the captured step and its cache key, EOS ids, stop
 * sequence, logits processors, token constraint, the draws keyed by (seed, row, step). */
int opus_generate_scored_behind(opus_ctx *ctx, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                const int32_t *h_lens, const int32_t *h_src, int32_t max_new, const int32_t *eos_ids, int32_t n_eos,
                                int32_t pad_id, float temperature, float top_p, uint64_t seed, int32_t *d_out_ids, int32_t *n_out,
                                float *d_token_logprobs, float *d_scores, float *d_logits, void *stream);
/* opus_llama_score_continuations / opus_llama_score_tree behind a snapshot instead of the context's current prefill: the same pass
 * with the attention reading d_k / d_v (no epoch, P = snap->P; d_last_rows fp32 [P, H] as opus_llama_prefix returned them).  Write
 * nothing but their outputs. */
int opus_llama_score_continuations_detached(opus_ctx *ctx, const opus_prefix_snap *snap, const void *d_embeds, int32_t R, int32_t n,
                                            const int32_t *h_lens, const int32_t *h_src, const float *d_last_rows,
                                            const int32_t *d_targets, float *d_logprob, void *d_scratch, int64_t scratch_bytes,
                                            void *stream);
int opus_llama_score_tree_detached(opus_ctx *ctx, const opus_prefix_snap *snap, const void *d_embeds, int32_t rows,
                                   const int32_t *h_src, const int32_t *h_par, const int32_t *h_depth, int32_t n_score,
                                   const int32_t *h_score_src, int32_t n_edges, const int32_t *h_edge_row, const int32_t *h_edge_tok,
                                   const int32_t *h_edge_slot, int32_t n_stops, const int32_t *h_stop_row, const int32_t *h_stop_set,
                                   const int32_t *h_stop_slot, int32_t n_stop_ids, const int32_t *h_stop_ids, int32_t n_stop_sets,
                                   const int32_t *h_stop_off, const float *d_last_rows, float *d_node_lp, float *d_stop_lp,
                                   int64_t n_slots, void *d_scratch, int64_t scratch_bytes, void *stream);

/* Prompt-lookup decoding (generate(prompt_lookup_num_tokens=k); transformers' PromptLookupCandidateGenerator + assisted decoding,
 * greedy and exact: the ids are those of opus_generate_greedy).  Added within ABI 10 (new symbols only).
 *   History of row b: d_hist[b, 0 .. h_hist_len[b]) (int32 [B, Lh], device; the caller's prompt ids without padding, -1 at every
 *     position a protein block was spliced into, then optionally -1 and a corpus to search) followed by the ids generated so far.
 *   Draft: for m from min(max_ngram, len - 1) down to 1, the FIRST window start i with h[i .. i + m) == h[len - m .. len), i + m < len
 *     and h[i + m] != -1; the draft is h[i + m .. min(i + m + k, len)), cut in front of a -1.  A window holding -1 never matches.
 *   Pass: n = 1 + the longest draft of an unfinished row (cut to the token budget) positions per row - the last committed id, whose
 *     K / V are not cached yet, then the draft (shorter drafts padded; the filler never counts as a match) - run through the
 *     prefill's layer loop behind the context's own cache (attn_prefix_kernel; the weights stream through the decode-class GEMM
 *     kernels, FP8 panels where bound), then the final norm and lm_head on all B n rows.  B (k + 1) <= max_batch, else OPUS_ESHAPE.
 *   Acceptance in lockstep: y_j the arg-max at position j, m_b the longest accepted prefix of row b's draft, a = min m_b over the
 *     unfinished rows; every row commits y_0 .. y_a and the step word advances by a + 1 (all rows stay at one cache slot).  An EOS id
 *     or the stop sequence among a row's COMMITTED ids finishes it there; pad behind.  No unfinished row has a draft: a plain decode step.
 * One stream synchronisation per pass.  stats (optional): {passes, plain steps, ids drafted, ids accepted}.  OPUS_EUNSUPPORTED with
 * logits processors or a token constraint set on the context; max_ngram in [1, 8]; B <= 64. */
int opus_generate_lookup(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                         const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, int32_t k, int32_t max_ngram, const int32_t *d_hist,
                         int32_t Lh, const int32_t *h_hist_len, int32_t *d_out_ids, int32_t *n_out, int64_t *stats, void *stream);
/* One verify pass with the caller's tokens on the current decode state (R = the rows of the last prefill, step word S): d_tokens
 * int32 [R, n] (device; column 0 the token whose K / V are not cached yet, then the draft), d_draft_len int32 [R] (device) or NULL
 * (n - 1 for every row).  Positions j = 0 .. n - 1 run at slots T0 + S + j; d_logits_all fp32 [R n, V] (row r n + j; optional),
 * d_argmax int32 [R, n] (optional).  *a (HOST) = the lockstep acceptance; the step word advances by a + 1, so that
 * opus_llama_decode_step or another verify step continues behind the accepted positions.  No ids are committed and no row ends.
 * Synchronises `stream`.  OPUS_ESHAPE: R n > max_batch, S + n > max_new_tokens, R > 64; OPUS_ESTATE without a prefill. */
int opus_llama_verify_step(opus_ctx *ctx, const int32_t *d_tokens, int32_t n, const int32_t *d_draft_len, float *d_logits_all,
                           int32_t *d_argmax, int32_t *a, void *stream);
/* Diagnostic: lookup_draft_kernel alone on R histories d_hist [R, Lh] of d_hist_len [R] ids (both device): d_draft int32 [R, k]
 * (0 behind the draft), d_draft_len [R]. */
int opus_debug_lookup_draft(opus_ctx *ctx, const int32_t *d_hist, int32_t Lh, const int32_t *d_hist_len, int32_t R, int32_t k,
                            int32_t max_ngram, int32_t *d_draft, int32_t *d_draft_len, void *stream);
/* Diagnostic: the projection buffer as the last attention launch of the context read it - operand dtype [rows, (heads + 2 kv) hd],
 * q | k | v of the LAST layer, q and k rotated (behind opus_llama_verify_step: row r n + j = position j of row r). */
int opus_debug_last_qkv(opus_ctx *ctx, void *d_out, int32_t rows, void *stream);
/* Diagnostic: lookup_accept_kernel alone. d_argmax / d_tokens int32 [R, n], d_draft_len [R] or NULL, the id matrix d_ids [R, stride],
 * d_fin [R], the step word d_step [1], d_next [R], d_nunf [stride] (all device, updated in place); pre = 1: a verify pass (commit at
 * columns step + 1 .., step += a + 1), pre = 0: behind a plain step (n = 1, commit at column step).  eos_ids / stop_ids: HOST arrays.
 * h_words (HOST) [4] = {a, rows unfinished, step word, ids drafted by unfinished rows}.  Synchronises `stream`. */
int opus_debug_lookup_accept(opus_ctx *ctx, const int32_t *d_argmax, const int32_t *d_tokens, const int32_t *d_draft_len, int32_t R,
                             int32_t n, int32_t pre, int32_t *d_ids, int32_t stride, int32_t *d_fin, int32_t *d_step,
                             const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, const int32_t *stop_ids, int32_t n_stop,
                             int32_t *d_next, int32_t *d_nunf, int32_t *h_words, void *stream);

/* Diagnostic: opus_generate_scored's fused arg-max / log-sum-exp pass on fp32 logits [B, V] (B <= max_batch, any V >= 1; rows
 * need no alignment): d_idx [B] the arg-max (lowest index among ties, bitwise what the greedy step picks), d_lse [B]. */
int opus_debug_argmax_lse(opus_ctx *ctx, const float *d_logits, int32_t B, int32_t V, int32_t *d_idx, float *d_lse, void *stream);
/* Top log-probs: the k likeliest tokens of a raw logits row l[0..V) and their log-probabilities.  Entries are ordered by value
 * descending, then index ascending - np.argsort(-l, kind="stable")[:k], an exact comparison of the stored values (-0 == +0); -inf
 * entries order like any value and give -inf; a row without a finite entry, and NaNs, are undefined.  top_lp[j] = l[top_ids[j]] -
 * lse(l) in fp32, the lse being the one d_token_logprobs uses.
 * opus_set_gen_top_logprobs(ctx, k, d_top_ids, d_top_lp), 1 <= k <= min(20, dec_vocab), applies to every later
 * opus_generate_scored / _fanout / _guided / _behind call of the context AND to opus_llama_forward, until cleared with k = 0 (the
 * buffers are then ignored); the setter launches nothing.
 *   generate: d_top_ids int32 / d_top_lp fp32 [rows, max_new, k], rows as the call's other outputs (B nret; P under guidance).  The
 *   row is the raw one: before guidance (the conditional row), the logits processors, the token constraint, temperature and the
 *   warpers.  A row that had finished before a step gets ids -1 and log-probs 0 at it (the step that emits the EOS id or the last
 *   stop-sequence id still counts); steps past *n_out are not written.  "On" is part of the captured step's identity, k and the
 *   addresses are not (they travel in the device descriptor): another k or fresh buffers instantiate no graph.  Off: every launch,
 *   graph and id is what it was.
 *   forward: [R, k] in the order of d_rows, from each lm_head chunk's 16-bit logits and the log-sum-exp of its NLL pass.
 * OPUS_EBADARG: k outside 0..20 or above dec_vocab, a NULL buffer with k > 0.  Added within ABI 10 (new symbols only). */
int opus_set_gen_top_logprobs(opus_ctx *ctx, int32_t k, int32_t *d_top_ids, float *d_top_lp);
/* Diagnostic: the two top-k launches alone on caller rows d_logits [R, ld] (dtype OPUS_F32, or OPUS_F16 = the build's 16-bit type;
 * V <= ld values a row; any R >= 1; rows need no alignment), 1 <= k <= min(20, V): d_ids int32 / d_lp fp32 [R, k].  d_lse fp32 [R],
 * or NULL: the rows' log-sum-exp is computed here (contiguous fp32 rows: by the decode step's fused arg-max / log-sum-exp pass). */
int opus_debug_top_logprobs(opus_ctx *ctx, const void *d_logits, int32_t dtype, int64_t ld, int32_t R, int32_t V, int32_t k,
                            const float *d_lse, int32_t *d_ids, float *d_lp, void *stream);
/* Diagnostic: the guidance launches of opus_generate_scored_guided alone on caller memory - fp32 logits [2 P, V] (any P >= 1, any
 * V >= 1; rows need no alignment): rows [0, P) become g (lsm(l_b) - lsm(l_{P+b})) + lsm(l_{P+b}) with lsm(x) = (x - max x) -
 * log(sum exp(x - max x)) in fp32 (g = 0 returns the partner rows' log-softmax as the kernel takes it); rows [P, 2 P) are not
 * written.  Added within ABI 10. */
int opus_debug_guidance(opus_ctx *ctx, float *d_logits, int32_t P, int32_t V, float guidance_scale, void *stream);

/* generate()'s logits processors, transformers' semantics and order (GenerationMixin._get_logits_processor): the repetition
 * penalty, no_repeat_ngram_size, bad_words_ids, then min_new_tokens; under sampling the temperature / top-k / top-p warpers follow.
 * The setting applies to the opus_generate_greedy / _sample / _scored calls of this context that follow (not to beam search),
 * until it is set again; all defaults (1.0, 0, 0, no entries) clear it, and the calls are then exactly those without processors.
 *   repetition_penalty p > 0 (1: off): every DISTINCT id of the row's history is changed once, s < 0 ? s * p : s / p (fp32).
 *   no_repeat_ngram_size n >= 0 (0: off): with t >= n - 1 ids generated, the id that followed each earlier occurrence of the last
 *     n - 1 ids is -inf.
 *   min_new_tokens m >= 0 (0: off): the call's EOS ids are -inf while fewer than m ids have been generated (no EOS ids: no-op).
 *   bad words (HOST arrays): entry e = bad_ids[bad_offsets[e] .. bad_offsets[e + 1]), n_bad + 1 offsets from 0.  A single id is
 *     -inf at every step unless it is one of the call's EOS ids (transformers drops such entries); the last id of a longer entry
 *     is -inf when the history is at least as long as the entry and ends with its other ids.  Ids lie in [0, dec_vocab).
 * The history is the ids generated so far, never the prompt (the reference generates from inputs_embeds); a finished row's
 * history holds its pad ids.  Capacities: at most 256 bad-word entries of 1 to 8 ids, 1024 ids in all; max_new <= 2048.
 * With processors on, opus_generate_scored's d_scores hold the processed scores; d_logits and d_token_logprobs stay raw (the
 * log-probability under the unprocessed distribution).  Only "on / off" is part of the captured step's identity: new values
 * need no new graph.  Returns OPUS_EBADARG for a value out of range or over a capacity. */
int opus_set_logits_processors(opus_ctx *ctx, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_new_tokens,
                               const int32_t *bad_ids, const int32_t *bad_offsets, int32_t n_bad);
/* Diagnostic: the processor kernel alone, in place on fp32 logits [B, V] (any B >= 1, V >= 1): row b's history is
 * d_hist[b * hist_stride + 0 .. hist_len) (device; hist_len <= 2048), eos_ids a HOST array (at most 64), the setting as above
 * (bad ids bounded by V).  Ordered on `stream`. */
int opus_debug_logits_process(opus_ctx *ctx, float *d_logits, int32_t B, int32_t V, const int32_t *d_hist, int32_t hist_stride,
                              int32_t hist_len, const int32_t *eos_ids, int32_t n_eos, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_new_tokens, const int32_t *bad_ids,
                              const int32_t *bad_offsets, int32_t n_bad, void *stream);

/* Constrained decoding: generate(prefix_allowed_tokens_fn=TokenTrie), transformers' PrefixConstrainedLogitsProcessor with a
 * deterministic token automaton instead of a Python callback.  It applies to the opus_generate_greedy / _sample / _scored calls
 * of this context that follow (not to beam search) until it is set again; n_states = 0 turns it off, and the calls are then
 * exactly those without it.  Behind min_new_tokens, in front of the sampling warpers.
 *   The table (HOST arrays, copied to a device allocation the context owns, outside the workspace; the call returns when the
 *   arrays are the caller's again): state s allows the ids edge_tok[edge_off[s] .. edge_off[s + 1]) (ascending within a state;
 *   n_states + 1 offsets from 0 to n_edges) and moves to edge_next[e] on edge e; a state with completing[s] != 0 allows the
 *   n_end end ids (1 to 64) too.  State 0 is the end state (no edges, completing): a row goes there on an end id and on any id
 *   its state did not allow (a finished row's pads), and may then only emit end ids.  Every other state allows something.
 *   start: n_start = 1 (every row starts there) or one start state per row (n_start = the batch of the generate calls; with
 *     opus_generate_scored_fanout: one per PROMPT, decoder row r starting at start[r / nret]).
 * Per step and row the kernel takes one transition on the id generated last (no walk over the history) and stores -inf to every
 * logit outside the allowed set; allowed logits are not touched.  d_scores of opus_generate_scored hold the masked scores,
 * d_logits and d_token_logprobs stay raw.  Only "on / off" is part of the captured step's identity: another table, other start
 * states need no new graph.  Returns OPUS_EBADARG for a table that is not well formed (offsets, ids outside [0, dec_vocab),
 * targets, order, a state that allows nothing). */
int opus_set_token_constraint(opus_ctx *ctx, int32_t n_states, const int32_t *edge_off, const int32_t *edge_tok,
                              const int32_t *edge_next, int32_t n_edges, const uint8_t *completing, const int32_t *end_ids,
                              int32_t n_end, const int32_t *start, int32_t n_start, void *stream);
/* Diagnostic: the constraint kernel alone, in place on fp32 logits [B, V] (B <= max_batch, any V >= 1 above the table's ids; rows
 * need no alignment), against the table set last: row b's history is d_hist[b * hist_stride + 0 .. hist_len) (device).  The rows'
 * states are brought to the end of the history by the kernel's own transition, one launch per id, and copied to d_state_out [B]
 * (device, optional).  Ordered on `stream`. */
int opus_debug_token_constraint(opus_ctx *ctx, float *d_logits, int32_t B, int32_t V, const int32_t *d_hist, int32_t hist_stride,
                                int32_t hist_len, int32_t *d_state_out, void *stream);

/* Diagnostic entry points (kernel-level parity tests and micro-benchmarks; not part of the path's
 * drop-in surface).  opus_debug_gemm: C[M,Nout] = epi(A[M,K] W[N,K]^T + bias) (+ residual fp32);
 * epi 0 none, 1 erf-GELU, 2 silu(gate)*up with W rows in [16 gate | 16 up] groups (Nout = N/2).
 * opus_debug_attention: softmax(scale * Q K^T + mask) V over [B,T,heads*hd] fp16 tensors
 * (K,V have heads/group heads); keys visible iff kstart[b] <= j < kend[b] (NULL = 0 / T) and
 * (!causal || j <= i). */
int opus_debug_gemm(opus_ctx *ctx, const void *d_A, const void *d_W, const float *d_bias, const float *d_residual,
                    void *d_C, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t out_f32, void *stream);
/* Same with the fused RMSNorm prologue: A is fp32 [M,K], C = epi(rmsnorm(A) W^T) (norm weight folded in W). */
int opus_debug_gemm_norm(opus_ctx *ctx, const float *d_A, const void *d_W, void *d_C, int32_t M, int32_t N, int32_t K,
                         int32_t epi, int32_t out_f32, float eps, void *stream);
/* The QKV projection of the batched decode step as decode_step issues it (5..64 rows, narrow output, k-parts leave raw fp32
 * slabs that the attention kernel sums): d_slabs fp32 [*ks][M][N] receives them, *ks (HOST) their number; *ks = 1: the launch
 * wrote a finished output instead and nothing is copied. */
int opus_debug_gemm_slabs(opus_ctx *ctx, const void *d_A, const void *d_W, float *d_slabs, int32_t M, int32_t N, int32_t K,
                          int32_t *ks, void *stream);
/* What the launchers launched for the last GEMM issued on this context (opus_debug_gemm, opus_debug_gemm_norm,
 * opus_debug_gemm_slabs, or a path call): plan (HOST) receives 8 ints - [0] kernel class (index into the class list of
 * opus_timing_names), [1] row-tile template argument (MT; TM of the ring kernel; 0: none), [2], [3] TN, NS of the ring kernel,
 * [4] the skinny kernel's LDS-staged-activation flag, [5] panels per workgroup of gemm_stream_kernel, [6] k-parts over workgroups
 * (big tiled GEMM: per tail tile), [7] how they become the output: 0 one k-part, 1 splitk_reduce_kernel, 2 splitk_reduce4_kernel,
 * 3 inside the launch (gemm_stream_kernel), 4 the big tiled GEMM's pair hand-off, 5 pp_tail_reduce_kernel, 6 raw slabs left
 * (opus_debug_gemm_slabs).  All -1: no GEMM yet, or the launcher refused the last one.  Added within ABI 10 (a new symbol only). */
int opus_debug_gemm_plan(opus_ctx *ctx, int32_t *plan);
/* opus_debug_gemm (form 0), opus_debug_gemm_norm (form 1: d_A fp32, eps; no bias / residual) or opus_debug_gemm_slabs (form 2: d_C
 * the slab buffer or NULL, *ks) with the FP8 form of W (opus_quantize_fp8: d_q8, d_e8) offered beside the panel-tiled d_W that holds
 * the same values, as the decode step offers it.  Routing is that of the plain entries; *ran_w8 (HOST) = 1 when the routed kernel
 * streamed the FP8 panels, 0 when it has no FP8 form and read d_W.  Added within ABI 10 (a new symbol only). */
int opus_debug_gemm_w8(opus_ctx *ctx, int32_t form, const void *d_A, const void *d_W, const void *d_q8, const void *d_e8,
                       const float *d_bias, const float *d_residual, void *d_C, int32_t M, int32_t N, int32_t K, int32_t epi,
                       int32_t out_f32, float eps, int32_t *ks, int32_t *ran_w8, void *stream);
/* opus_debug_gemm_w8 with the MXFP4 form of W (opus_quantize_mxfp4: d_q4, d_s4) in the place of the FP8 form; *ran_w4 (HOST) = 1
 * when the routed kernel streamed the MXFP4 panels.  Added within ABI 10 (a new symbol only). */
int opus_debug_gemm_w4(opus_ctx *ctx, int32_t form, const void *d_A, const void *d_W, const void *d_q4, const void *d_s4,
                       const float *d_bias, const float *d_residual, void *d_C, int32_t M, int32_t N, int32_t K, int32_t epi,
                       int32_t out_f32, float eps, int32_t *ks, int32_t *ran_w4, void *stream);
/* Process-wide tuning knob of the benchmarks / parity tests (no reference counterpart): "no_stream" = 1 routes the narrow
 * GEMMs of the batched decode step through the round-2 split-K kernels instead of gemm_stream_kernel; "pp_gm" = tile rows
 * per rasterisation group of the big tiled GEMM; "debug_a_tiled" = 1: opus_debug_gemm takes A in fragment order; "no_ln_fusion" = 1: stand-alone normalisation kernels
 * instead of the norms fused around the big tiled GEMM; "enc_full_last_layer" = 1: the token-packed encoder's last layer computes
 * the <cls> / <eos> rows as well; "poison_handoff" = 1 (needs ctx): leaves the hand-off words as an
 * aborted launch would (test aid); "misc0".."misc7" scratch.  ctx (may be NULL) drops its captured decode graph. */
int opus_debug_knob(opus_ctx *ctx, const char *name, int32_t value);
/* The row-scale RMSNorm fusion as the decoder issues it (api.cpp prefill / decode_step): X <- X + A W1^T through a GEMM
 * (gemm_stream_kernel at 5..64 rows, else a split-K GEMM) whose epilogue / reduce also writes fp16(X) and per-block sums of squares, then C = epi(rmsnorm(X) W2^T) with
 * the rows scaled inside the consumer GEMM.  A fp16 [M,K1], W1 [N1,K1] and W2 [N2,N1] panel-tiled, X fp32 [M,N1] in/out,
 * C fp16 [M, N2 or N2/2]; *fused (HOST) = 1 when the fused kernels ran. */
int opus_debug_gemm_rowscale(opus_ctx *ctx, const void *d_A, const void *d_W1, float *d_X, const void *d_W2, void *d_C,
                             int32_t M, int32_t N1, int32_t K1, int32_t N2, int32_t epi, float eps, int32_t *fused,
                             void *stream);
/* The ESM-2 QKV projection + rotary as opus_esm2_encode issues it: out[M, 3 D] fp16 = rotary(A[M,K] W[3 D,K]^T + bias), query
 * third scaled by head_dim^-0.5 before the rotation, position of row m = m % T (cstp_v3 / modeling_esm.py:374, rotary
 * embedding).  The context's encoder head_dim must equal D / heads.  allow_fuse = 0 forces the stand-alone rotary kernel on
 * the stored projection; *fused (HOST) = 1 when the rotation ran in the GEMM's epilogue (large M, head_dim 64). */
int opus_debug_gemm_rope(opus_ctx *ctx, const void *d_A, const void *d_W, const float *d_bias, void *d_out, int32_t M,
                         int32_t D, int32_t K, int32_t T, int32_t heads, int32_t allow_fuse, int32_t *fused, void *stream);
/* The LayerNorm / RMSNorm fused around the big tiled GEMM as opus_esm2_encode (pre-LN blocks, modeling_esm.py EsmLayer) and
 * opus_llama_prefill (LlamaRMSNorm) issue it, three steps:
 *   X <- X + A W1^T (+ b1)   fp32 [M,N1] in place; the GEMM also writes fp16(X) to d_xh [M,N1] and, per row and 64-column slab,
 *                            (sum x, sum x^2) to d_part [M, N1/64, 2]
 *   d_stat [M,2] = (mu, rstd) of every row from the partials (rms != 0: (0, rsqrt(mean x^2 + eps)))
 *   C = epi(rstd (fp16(X) W2^T - mu s) + c2)   fp16 [M, N2 or N2/2]: W2 = W diag(gamma) [N2,N1], d_c2 = W beta + b (or NULL),
 *                            d_colsum s[n] = sum_k W2[n][k] (LayerNorm; NULL with rms); epi 0 / 1 (GELU) / 2 (gate-up, rms only).
 * rope_T > 0 (epi 0, N2 = 3 D, head_dim 64): the ESM rotary runs in the consumer's epilogue as in opus_debug_gemm_rope, row m at
 * position m % rope_T or, with d_rope_pos int32 [M] (token-packed batches), d_rope_pos[m].  A fp16 [M,K1]; W1, W2 panel-tiled.
 * d_part / d_xh / d_stat are the caller's.  *produced (HOST) = 1 when the first GEMM left the partials; 0: its shape is off the
 * fused form, nothing further ran (no stand-alone fallback).  plan (HOST, int32[10]): what the big tiled GEMM launched for the
 * first ([0..5)) and the second ([5..10)) GEMM - whole-K tiles, tail tiles cut into k-parts, parts per tail tile, combine
 * (0 none, 1 pair inside the launch, 2 reduce kernel), rotary fused; -1 where that kernel did not run. */
int opus_debug_gemm_ln(opus_ctx *ctx, const void *d_A, const void *d_W1, const float *d_b1, float *d_X, float *d_part, void *d_xh,
                       float *d_stat, const void *d_W2, const float *d_c2, const float *d_colsum, void *d_C, int32_t M, int32_t N1,
                       int32_t K1, int32_t N2, int32_t epi, int32_t rms, float eps, int32_t rope_T, const int32_t *d_rope_pos,
                       int32_t *produced, int32_t *plan, void *stream);
int opus_debug_attention(opus_ctx *ctx, const void *d_Q, const void *d_K, const void *d_V, void *d_O,
                         const int32_t *d_kstart, const int32_t *d_kend, int32_t B, int32_t T, int32_t heads,
                         int32_t group, int32_t head_dim, int32_t causal, float scale, void *stream);

/* attn_prefill_kernel launched as opus_esm2_encode* / opus_llama_prefill launch it: one launch, the caller's pointers and strides
 * as they stand, no buffer of the context involved.  Element (b, t, head h, d) of Q is d_Q[b * q_sb + t * q_st + h * head_dim + d]
 * (K / V: kv head h / group; O likewise with o_sb / o_st), strides in 16-bit elements - so Q / K / V may be column ranges of one
 * fused projection buffer ([rows, 3 D] of the encoder, [rows, (heads + 2 kv) head_dim] of the decoder).  Three forms:
 *   padded        d_cu NULL: B rows of T tokens, key j of row b visible iff d_kstart[b] <= j < d_kend[b] (NULL = 0 / T) and
 *                 (!causal || j <= i); a query without a visible key gives zeros;
 *   token-packed  d_cu int32 [B + 1] (device): row b = tokens d_cu[b] .. d_cu[b + 1] - 1 of the buffers, all of them keys and
 *                 queries; T = the longest row; batch strides, d_kstart and d_kend are ignored; causal must be 0
 *                 (OPUS_EUNSUPPORTED otherwise: the path has no such form);
 *   ... q_trim    token-packed with q_trim = 1 (T > 2): the first and the last token of every row are keys but not queries,
 *                 their rows of O are left as they were.
 * *qt_used (HOST) = the 16-query tiles per wave the launcher chose (1 or 2; knob "misc3" = 1 swaps the choice); 0 when nothing
 * was launched.  Errors: OPUS_EBADARG for a null ctx / Q / K / V / O / qt_used, OPUS_ESHAPE for B, T, heads, group < 1, heads
 * not a multiple of group, a stride < 1 or q_trim without d_cu or with T <= 2 - all before any device call; OPUS_EHIP, with no
 * launch, where the launcher refuses: a q / k / v stride that is no multiple of 8 elements (o: 4), T * max(k_st, v_st) * 2 >= 2^31
 * bytes (32-bit buffer offsets), head_dim other than 16 / 32 / 64 / 128. */
int opus_debug_attn_prefill(opus_ctx *ctx, const void *d_Q, const void *d_K, const void *d_V, void *d_O, int64_t q_st, int64_t k_st,
                            int64_t v_st, int64_t o_st, int64_t q_sb, int64_t k_sb, int64_t v_sb, int64_t o_sb,
                            const int32_t *d_kstart, const int32_t *d_kend, const int32_t *d_cu, int32_t B, int32_t T,
                            int32_t heads, int32_t group, int32_t head_dim, int32_t causal, int32_t q_trim, float scale,
                            int32_t *qt_used, void *stream);

/* attn_decode_kernel as opus_llama_decode_step launches it, alone, on layer 0 of this context's KV cache (kernel-level parity
 * of rows D3 / D4 at any cache length: transformers' eager attention over a cache, modeling_llama.py:191-213, reached from
 * language_model/opus_llama.py:127).  d_qkv fp16 [B, (heads + 2 kv) hd]: the new token's q | k | v projections, not yet rotated;
 * d_k_hist / d_v_hist fp16 [B, kv, L, hd], L = T0 + step: the cache contents of slots 0 .. L-1 (keys rotated); d_kstart int32
 * [B]: first visible slot of each (left-padded) row.  The new token sits at slot L, position L - kstart[b].
 * d_out fp16 [B, heads hd]; d_k_new / d_v_new (optional) fp16 [B, kv, hd]: slot L of the cache afterwards.
 * Overwrites the cache of the last prefill (opus_llama_decode_step then fails with OPUS_ESTATE until the next prefill). */
int opus_debug_attn_decode(opus_ctx *ctx, const void *d_qkv, const void *d_k_hist, const void *d_v_hist, const int32_t *d_kstart,
                           int32_t B, int32_t T0, int32_t step, void *d_out, void *d_k_new, void *d_v_new, void *stream);

/* The same single launch in every form opus_llama_decode_step gives attn_decode_kernel.  The input is EITHER d_qkv (as above) OR
 * the fused form of 4 < B <= 64: d_slabs fp32 [ks, B, (heads + 2 kv) hd], the raw k-part slabs of the QKV GEMM (ks = 1 .. 8), with
 * d_row_ssq fp32 [B, row_nblk] - the sums of squares of the GEMM's input rows in blocks, over K columns in all -, eps and an
 * optional d_bias fp32 [(heads + 2 kv) hd]: the kernel itself forms (sum of slabs) * rsqrt(sum(row_ssq[b]) / K + eps) + bias and
 * rounds it to the operand type before the rotary.  All of them the caller's pointers as they stand.  out_tiled = 1: d_out holds
 * 16 ceil(B / 16) rows in the fragment order a tiled-A GEMM reads (csrc/common.h tiled_off); rows >= B are not written.
 * d_k_cache / d_v_cache (optional) [B, kv, max_prompt + max_new_tokens, hd]: layer 0's whole cache after the launch.
 * *gp_used (HOST) = the query heads per workgroup the launcher chose (1 = one workgroup per head, 2 / 4 / 8 = per kv group);
 * 0 when nothing was launched.  Errors, all before any device call: OPUS_EBADARG for a null ctx / d_kstart / d_out / gp_used /
 * history and for both or neither of d_qkv / d_slabs; OPUS_ESHAPE for B, T0, step outside the context, ks outside 1 .. 8,
 * row_nblk < 1 or K < 1, slabs without d_row_ssq, out_tiled with heads * hd not a multiple of 64. */
int opus_debug_attn_decode_form(opus_ctx *ctx, const void *d_qkv, const float *d_slabs, int32_t ks, const float *d_row_ssq,
                                int32_t row_nblk, int32_t K, float eps, const float *d_bias, const void *d_k_hist,
                                const void *d_v_hist, const int32_t *d_kstart, int32_t B, int32_t T0, int32_t step,
                                int32_t out_tiled, void *d_out, void *d_k_new, void *d_v_new, void *d_k_cache, void *d_v_cache,
                                int32_t *gp_used, void *stream);

/* Synchronises `stream` and returns OPUS_EHIP if an in-launch split-K hand-off of this context gave up waiting since the last
 * check (see Conventions; the results of the calls in between are invalid), OPUS_OK otherwise.  opus_generate_* make the same
 * check before they return.  No reference counterpart (torch raises asynchronously on device-side faults). */
int opus_check_error(opus_ctx *ctx, void *stream);

/* Row N1, `num_beams` (eval/run_opus_ddp.py:129,158 -> transformers GenerationMixin._beam_search).  The decoder runs B x K rows
 * (row = b K + k) through opus_llama_prefill / opus_llama_decode_step; these two do the per-step work that touches O(K V) values or
 * the KV cache, the caller keeps the O(K) bookkeeping of running / finished beams (opus-pllm_amd/beam.py, as the reference's
 * Python does).
 * opus_beam_topk: over the fp32 logits of this context's last step, scores fp32 [B, M] (descending; ties: lower index first)
 *   and flat indices k * dec_vocab + token int32 [B, M] of the M best values of log_softmax(logits[b K + k]) + run_scores[b K + k]
 *   (generation/utils.py _get_top_k_continuations; M = max(2, 1 + #eos) K <= 16).
 * opus_kv_reorder: KV cache rows r <- rows d_src_rows[r] in every layer (Cache.reorder_cache(beam_idx)); R = rows of the last prefill. */
int opus_beam_topk(opus_ctx *ctx, const float *d_run_scores, int32_t B, int32_t K, int32_t M, float *d_scores, int32_t *d_idx,
                   void *stream);
int opus_kv_reorder(opus_ctx *ctx, const int32_t *d_src_rows, int32_t R, void *stream);
/* Beam-sample (`num_beams` > 1 with temperature > 0: run_opus_ddp.py:126-129 passes both; _get_top_k_continuations' do_sample
 * branch = torch.multinomial(softmax(accumulated), M), without replacement).  Per decoder row: log_softmax, then the warpers on
 * the log-probabilities (temperature, top_k of opus_set_sampling_top_k, top_p - both with min_tokens_to_keep = M / K, i.e. #eos + 1
 * and at least 2, as GenerationMixin._get_logits_processor builds them when num_beams > 1); per batch row: M continuations drawn without
 * replacement from softmax over the K rows' kept values + run_scores.  d_scores fp32 [B, M] = the accumulated log-probabilities of
 * the draws, d_idx int32 [B, M] = k * dec_vocab + token, in the order drawn; entries beyond the continuations of non-zero
 * probability are -inf / 0x7fffffff (torch.multinomial raises there: the caller should).  Draws come from a counter-based generator
 * keyed by (seed, step, row, token): distributional parity, reproducible per seed.  d_logits NULL = this context's last step. */
int opus_beam_sample_topk(opus_ctx *ctx, const float *d_logits, const float *d_run_scores, int32_t B, int32_t K, int32_t M,
                          float temperature, float top_p, uint64_t seed, int32_t step, float *d_scores, int32_t *d_idx, void *stream);
/* TopKLogitsWarper of this context's sampling paths (opus_generate_sample, opus_debug_sample, opus_beam_sample_topk), between the
 * temperature and the nucleus: k > 0 keeps the k most probable tokens and whatever ties with the k-th; 0 (the state of a new
 * context) = off.  transformers 4.46.3 - requirements.txt:20 of the reference - defaults GenerationConfig.top_k to 50 when it
 * samples (transformers >= 5: None); the Python mirror's generate(top_k=...) defaults to 50 accordingly. */
int opus_set_sampling_top_k(opus_ctx *ctx, int32_t k);
/* The truncation warpers of this context's sampling paths (opus_generate_sample, opus_generate_scored and its forms,
 * opus_debug_sample, the continuous-batching session), behind the temperature, top-k and top-p in transformers' order - MinP,
 * Typical, Epsilon, Eta, each with min_tokens_to_keep = 1 and each seeing the softmax over what the earlier ones kept.  With
 * p = exp(l / T - max / T) over the set K0 that top-k / top-p keep:
 *   min_p m:          keeps p >= m (m times the largest p, 1).
 *   typical_p t < 1:  q = p / Z, H = -sum q log q, d = |-log q - H|; keeps the smallest prefix in ascending d whose mass reaches t
 *                     (the token that crosses t stays, ties in d stay together): a band p_lo <= p <= p_hi around Z e^-H that can
 *                     leave the arg-max token out.
 *   epsilon_cutoff e: removes q < e (q over the survivors); every token at the survivors' maximum stays.
 *   eta_cutoff e':    the same with min(e', sqrt(e') e^-H), H over the survivors at that point.
 * The draw is the CDF inversion of opus_generate_sample over the band that is left, with the same (seed, row, step) uniform;
 * output_scores hold l / T on the band and -inf elsewhere.  Off values (a new context's state): 0, 1, 0, 0; with all four off every
 * launch and draw is what it was without this entry point.  The captured decode step reads the values from device memory: changing
 * them instantiates no graph.  OPUS_EBADARG outside min_p in [0, 1], typical_p in (0, 1], both cutoffs in [0, 1), and for a null
 * context (before the device is touched).  opus_beam_sample_topk returns OPUS_EUNSUPPORTED while any warper is on.  (Added within
 * ABI 10.) */
int opus_set_sampling_warpers(opus_ctx *ctx, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff);

/* Continuous batching (no reference counterpart; added within ABI 10): one live decode batch - a session - whose done rows are handed
 * to new prompts while the other rows keep decoding.  Step t of a session writes every row's token to column t of d_ids int32
 * [B, S] (S = max_new_tokens of the context: the session's step budget) and its K / V to cache slot T + t.  A row is done at the
 * first step at which it emitted an EOS id, completed the stop sequence, or has emitted max_new tokens since its occupant began.
 * opus_stream_begin: opus_generate_*'s checks, uploads and prefill (B rows, T left-padded positions); every row begins at step 0.
 *   OPUS_EUNSUPPORTED while logits processors or a token constraint are set.
 * opus_stream_run: at every step boundary t the host knows the rows' state as of step t - opus_stream_lag() (it never enqueues
 *   more than that ahead) and returns - *t_out = t, h_end[r] (HOST, int32 [B]) = the step row r was done at, -1 if not (yet, as far
 *   as known) - when every row is done, when t == t_max (at most S), or when t >= t_min and at least min_free rows are done;
 *   otherwise it enqueues step t (from a captured graph of its own: the plain decode graphs are neither used nor evicted).  What it
 *   returns is a function of the rows' end steps alone.
 * opus_stream_refill (at the boundary opus_stream_run returned): rows h_rows[i] (n of them, each once) take the prompts that were
 *   prefilled elsewhere: row h_src[i] of the detached snapshot, of h_len[i] = Tp - kstart slots, is placed at cache slots
 *   [T + t - h_len[i], T + t) of the row, whose kstart moves there; row h_src[i] of d_last_logits (fp32 [snap rows, dec_vocab]) becomes
 *   the row's logits; its flags are cleared, its occupant begins at step t, and id columns t - 8 .. t - 1 are set to -1 (the stop
 *   sequence is matched against at most 8 ids back).  No other row is touched.  OPUS_ESHAPE when a prompt does not fit under T + t
 *   slots or t + max_new > S.  Prefix handles of the context go stale.
 * opus_stream_end synchronises, fills h_end (optional, HOST int32 [B]) with the rows' end steps as of the last enqueued step and
 *   leaves the context as after opus_generate_*.  Any prefill on the context also ends a session. */
int32_t opus_stream_lag(void);
int opus_stream_begin(opus_ctx *ctx, const void *d_embeds, const uint8_t *d_mask, int32_t B, int32_t T, int32_t max_new,
                      const int32_t *eos_ids, int32_t n_eos, int32_t pad_id, float temperature, float top_p, uint64_t seed,
                      int32_t *d_ids, void *stream);
int opus_stream_run(opus_ctx *ctx, int32_t t_min, int32_t min_free, int32_t t_max, int32_t *t_out, int32_t *h_end, void *stream);
int opus_stream_refill(opus_ctx *ctx, const opus_prefix_snap *snap, int32_t n, const int32_t *h_rows, const int32_t *h_src,
                       const float *d_last_logits, const int32_t *h_len, void *stream);
int opus_stream_end(opus_ctx *ctx, int32_t *h_end, void *stream);
/* Test support: synchronises `stream`; kstart, finished flags, start and end steps (HOST, int32 [B] each) of the open session's rows
 * and the cache epoch (for opus_llama_prefix_export).  poison != 0: the whole KV cache is first filled with that byte. */
int opus_debug_stream_state(opus_ctx *ctx, int32_t *h_kstart, int32_t *h_fin, int32_t *h_start, int32_t *h_end, int64_t *epoch,
                            int32_t poison, void *stream);

/* fp32 logits [B, dec_vocab] of the most recent prefill / decode step (device copy on `stream`): the payload of the
 * optional logits all-gather of SURVEY 8e (ids are what eval/run_opus_ddp.py:138 gathers). */
int opus_last_logits(opus_ctx *ctx, float *d_out, int32_t B, void *stream);

/* Counters of a context (no reference counterpart; -1 for an unknown name).  "graph_instantiations": decode-step hipGraphs
 * instantiated since the context was created - the captured step reads the prompt length from device memory, so a dataset's
 * batches share one graph whatever their T (the reference's loop, eval/run_opus_ddp.py:88-135, brings a new T with every batch);
 * a different number of rows / token budget / sampling setting is another graph (a few are kept).  "graph_replays": decode steps
 * launched from a graph.  "graphs_cached".  "decode_steps": decode steps the generate loops enqueued - with an EOS id or a stop
 * sequence the loop polls the rows' state with a bounded run-ahead and stops at most 2 steps after the last row finished (HF stops
 * at once; the extra steps emit pad ids only, the returned ids and n_out are exact).  "w8_gemms": GEMMs issued on this context
 * (eagerly or while a graph was captured; replays are not counted) whose kernel streamed the FP8 panels.  "w4_gemms": the same for the MXFP4 panels.
 * "cache_epoch": the current cache epoch - what opus_llama_prefix_export takes, also behind an opus_generate_* call, which hands
 * none out. */
int64_t opus_stat(opus_ctx *ctx, const char *name);

/* Measurement support (bench.py).  With timing enabled (off by default; decode runs eagerly instead of from the
 * hipGraph) every kernel launch of the path is recorded with its own dispatch start / end events on the launch stream
 * (hipExtLaunchKernelGGL - the interval rocprofv3 --kernel-trace reports), its kernel class, the phase of the path it
 * belongs to, and its ALGORITHMIC bytes and FLOPs.  opus_timing_get sums the records since the last reset that match
 * kernel_class and phase ("*" = any); opus_timing_names returns "class,class,...;phase,phase,..." .  Classes and phases are
 * addressed by name, never by position.  Order of the lists: phases are append-only ("score" last); among the classes "xent"
 * stays the last entry, as published since opus_llama_forward, and a class added later ("contact", "trie_search", "topk", "constraint", "guidance", "mlm", "logitproc") is
 * listed in front of it ("constraint", "guidance", "mlm", "logitproc" keep their places next to "xent"). */
int opus_timing_enable(opus_ctx *ctx, int32_t on);
int opus_timing_reset(opus_ctx *ctx);
int opus_timing_get(opus_ctx *ctx, const char *kernel_class, const char *phase, double *ms, int64_t *launches, double *bytes,
                    double *flops);
int opus_timing_names(char *buf, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* OPUS_PLLM_H */
