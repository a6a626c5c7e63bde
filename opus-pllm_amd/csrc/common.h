// Shared declarations for libopus_pllm.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace opus {

// The 16-bit operand type of the build: IEEE fp16 (default: the reference's unquantised dtype, model/builder.py:57) or - with
// -DOPUS_BF16, build.py's second library libopus_pllm_bf16.so - bfloat16 (SURVEY 8(d) "bf16 switchable": Llama-3 checkpoints are
// bf16-native).  Every kernel is written against half_t / h8 and mfma16(); accumulation, residual stream, norms and softmax are
// fp32 in both builds.
#ifdef OPUS_BF16
typedef __bf16 half_t;
typedef __bf16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 h4 __attribute__((ext_vector_type(4)));
typedef __bf16 h2 __attribute__((ext_vector_type(2)));
#else
typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#endif
typedef float f4 __attribute__((ext_vector_type(4)));
// D = A (16 x 32) B (32 x 16) + C on the matrix cores, operands in the build's 16-bit type
__device__ __forceinline__ f4 mfma16(h8 a, h8 b, f4 c) {
#ifdef OPUS_BF16
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#endif
}

enum Epi { EPI_NONE = 0, EPI_GELU = 1, EPI_SILU_GU16 = 2 };
// first unit of k-part `part` of `parts` over `n` units (n * parts < 2^31): 32-bit, and free when there is one part - the
// 64-bit form of this was ~100 scalar instructions in front of the first load of every weight-streaming kernel
__device__ __forceinline__ int kpart_begin(int n, int part, int parts) {
    return parts == 1 ? (part ? n : 0) : (int)((unsigned)(n * part) / (unsigned)parts);
}
// Every GemmParams field a weight-streaming kernel reads before its first load, fetched in ONE scalar batch (the compiler
// otherwise loads the ~330-byte argument block piecemeal: up to six dependent scalar round trips before the first weight load)
#define OPUS_ARGS_ONE_BATCH(p)                                                                                                        \
    asm volatile("" ::"s"((p).A), "s"((p).Af), "s"((p).W), "s"((p).C), "s"((p).bias), "s"((p).residual), "s"((p).ws), "s"((p).xh_out),  \
                 "s"((p).ssq_out), "s"((p).row_ssq), "s"((p).lda), "s"((p).ldc), "s"((p).ldr), "s"((p).M), "s"((p).N), "s"((p).K),     \
                 "s"((p).out_f32), "s"((p).norm_eps), "s"((p).row_nblk), "s"((p).no_rot), "s"((p).c_tiled))
// M up to which the weight-streaming skinny kernel CAN be used (LDS-staged activations, fused RMSNorm); the mid / wide
// kernels take over above skinny_max_m().
constexpr int SKINNY_MAX_M_CAP = 16;
int skinny_max_m();   // rows up to which the skinny kernel is used (default 4, at most 16; OPUS_SKINNY_MAX_M tunes it)
#define SKINNY_MAX_M skinny_max_m()
// M up to which the mid kernel (LDS-shared activations, per-wave weight stream, fused RMSNorm) is used
constexpr int MID_MAX_M = 64;   // (65..128 rows measured faster on the split-K tile kernel)
// kernel classes of the per-launch timing (opus_timing_get): one per kernel family
enum KClass { KC_SKINNY = 0, KC_MID, KC_WIDE, KC_RING, KC_PP, KC_TILE, KC_REDUCE, KC_ATTN_PREFILL, KC_ATTN_DECODE, KC_NORM,
              KC_OTHER, KC_STREAM, KC_CONTACT, KC_TRIE_SEARCH, KC_TOPK, KC_CONSTRAINT, KC_GUIDANCE, KC_MLM, KC_LOGITPROC, KC_XENT, KC_COUNT };
// Ordering rule of the published class list (opus_timing_names, include/opus_pllm.h): "xent" stays its last entry, as published
// since opus_llama_forward, and a class added later goes in front of it.  Classes are looked up by name, never by index.
// phases of the path a launch belongs to (set by the entry points of api.cpp)
enum Phase { PH_ENCODE = 0, PH_PROJECT, PH_SPLICE, PH_PREFILL, PH_DECODE, PH_OTHER, PH_SCORE, PH_COUNT };

// Measurement hook.  While a LaunchEvents record is armed (thread-local, set by api.cpp in timing mode only), the next
// principal kernel launch is dispatched with hipExtLaunchKernelGGL so that (main0, main1) carry the dispatch's own start /
// end timestamps - the interval rocprofv3 --kernel-trace reports - and a split-K reduce launched behind it uses (aux0, aux1).
struct LaunchEvents {
    hipEvent_t main0 = nullptr, main1 = nullptr, aux0 = nullptr, aux1 = nullptr;
    int main_class = -1;
    bool main_used = false, aux_used = false;
    double aux_bytes = 0.0;
};
extern thread_local LaunchEvents *tl_launch_ev;
#define OPUS_LAUNCH(klass, kernel, grid, block, lds, stream, ...)                                                        \
    do {                                                                                                                  \
        ::opus::LaunchEvents *ev_ = ::opus::tl_launch_ev;                                                                 \
        if (ev_ && (klass) != ::opus::KC_REDUCE && !ev_->main_used) {                                                     \
            ev_->main_used = true;                                                                                        \
            ev_->main_class = (klass);                                                                                    \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_->main0, ev_->main1, 0, __VA_ARGS__);              \
        } else if (ev_ && (klass) == ::opus::KC_REDUCE && !ev_->aux_used) {                                               \
            ev_->aux_used = true;                                                                                         \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_->aux0, ev_->aux1, 0, __VA_ARGS__);                \
        } else {                                                                                                          \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                            \
        }                                                                                                                 \
    } while (0)
// hipFuncAttributeMaxDynamicSharedMemorySize, remembered per (device, kernel): a second device in the same process gets its own call
hipError_t ensure_dyn_lds(const void *fn, size_t bytes);

// C[M,Nout] = epi(A[M,K] * W[N,K]^T + bias) (+ residual).  fp16 operands, fp32 accumulate.
// EPI_SILU_GU16: W rows come in 32-row groups [16 gate | 16 up]; Nout = N/2, out = silu(g) * u.
// One rotary pair, with the contraction spelled out (one rounded product, one fused multiply-add) so that every kernel
// that rotates - the stand-alone kernels and the fused GEMM epilogue - produces the same bits from the same inputs.
// The results are pinned in fp32 registers: left to itself the compiler folds a following conversion to fp16 into the
// multiply-add (v_fma_mixlo_f16: ONE rounding, straight to fp16) in some kernels and not in others - a 1-ulp difference in
// 6e-5 of the elements; fp32 first, then fp16, is also what the reference's fp32 rotary followed by .to(fp16) does.
__device__ __forceinline__ void rotate_pair(float a, float b, float c, float sn, float &lo, float &hi) {
    lo = __builtin_fmaf(a, c, -__fmul_rn(b, sn));
    hi = __builtin_fmaf(b, c, __fmul_rn(a, sn));
    asm volatile("" : "+v"(lo), "+v"(hi));
}

// offset (in elements) of element (row, k) of a fragment-ordered [rows, K] fp16 matrix: 16-row x 64-k blocks of 2 KB in MFMA
// operand order [k-step][lane = 16 ((k % 32) / 8) + row % 16][8] - the panel-tiled weight layout with rows for output columns
__host__ __device__ __forceinline__ int64_t tiled_off(int row, int k, int K) {
    return ((int64_t)(row >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((k & 63) >> 5) * 512 + ((((k & 31) >> 3) << 4) + (row & 15)) * 8 + (k & 7);
}

// FP8 decoder weights (quant.hip, DESIGN section 4 "FP8 panels").  W[N][K] as OCP e4m3fn codes with one power-of-two exponent per
// row: block (p = n / 16, c = k / 64) is the 1 KB at ((p K / 64) + c) 1024 bytes; lane g 16 + li (n = 16 p + li) owns 16 bytes,
// bytes 0 .. 7 = k 64 c + 8 g + e (the first k-step of the chunk), bytes 8 .. 15 = k 64 c + 32 + 8 g + e (the second): one wave-wide
// 16-B load is 1 KB of contiguous HBM and, converted, both B operands of the chunk.
__host__ __device__ __forceinline__ int64_t fp8_tiled_off(int64_t n, int64_t k, int64_t K) {
    return ((n >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((((k & 31) >> 3) << 4) + (n & 15)) * 16 + ((k & 63) >> 5) * 8 + (k & 7);
}
constexpr int W8_EXP_MIN = -120;            // floor of the row exponents (int8, and 2^e stays a normal fp32)
#ifdef OPUS_BF16
constexpr int OPERAND_MIN_EXP = -126, OPERAND_MAX_EXP = 127;     // binary exponents of the smallest normal / largest finite operand
#else
constexpr int OPERAND_MIN_EXP = -14, OPERAND_MAX_EXP = 15;
#endif
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// 16 e4m3fn codes (one lane's 16 bytes of an FP8 panel block) -> the two B operands of the chunk, exactly: every code is a
// normal number (or zero) of either operand type (v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1)
__device__ __forceinline__ void fp8x16_to_h8(u32x4 q, h8 &lo, h8 &hi) {
#ifdef OPUS_BF16
#define OPUS_CVT_FP8(w, sel) __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)(w), 1.0f, sel)
#else
#define OPUS_CVT_FP8(w, sel) __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)(w), 1.0f, sel)
#endif
    const h2 a0 = OPUS_CVT_FP8(q[0], false), a1 = OPUS_CVT_FP8(q[0], true), a2 = OPUS_CVT_FP8(q[1], false), a3 = OPUS_CVT_FP8(q[1], true);
    const h2 b0 = OPUS_CVT_FP8(q[2], false), b1 = OPUS_CVT_FP8(q[2], true), b2 = OPUS_CVT_FP8(q[3], false), b3 = OPUS_CVT_FP8(q[3], true);
#undef OPUS_CVT_FP8
    lo = h8{a0[0], a0[1], a1[0], a1[1], a2[0], a2[1], a3[0], a3[1]};
    hi = h8{b0[0], b0[1], b1[0], b1[1], b2[0], b2[1], b3[0], b3[1]};
}
// 2^e of a row exponent (W8_EXP_MIN <= e <= 120)
__device__ __forceinline__ float exp2_i8(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }
// quant.hip: q8 (FP8 panels), e8 [N], dq (operand type, row-major [N, K]; may be null) from row-major src [N, K]; *bad (device,
// zeroed by the caller) is set when a weight is not finite
hipError_t launch_quantize_fp8(const half_t *src, int64_t N, int64_t K, uint8_t *q8, int8_t *e8, half_t *dq, int *bad, hipStream_t s);

// MXFP4 decoder weights (quant.hip, DESIGN section 4 "MXFP4 panels").  W[N][K] as OCP e2m1 codes (sign in bit 3, two per byte, the
// lower k in the low nibble) with one e8m0 scale byte per 32 consecutive k of a row.
// Code panels: block (p = n / 16, c = k / 64) is the 512 B at ((p K / 64) + c) 512; lane g 16 + li (n = 16 p + li) owns 8 bytes,
// bytes 0 .. 3 = k 64 c + 8 g + 0 .. 7 (the first k-step of the chunk), bytes 4 .. 7 = k 64 c + 32 + 8 g + 0 .. 7 (the second):
// one wave-wide 8-B load is 512 B of contiguous HBM.  Scale panels: block (p, c) is the 32 B at ((p K / 64) + c) 32, row li owns
// bytes 2 li (the first k-step's scale) and 2 li + 1 (the second's): one 2-B load per lane, 32 B of contiguous HBM per wave.
// mx4_code_off: the byte that holds element (n, k) (nibble k & 1); mx4_scale_off: the byte of (n, block kb = k / 32).
__host__ __device__ __forceinline__ int64_t mx4_code_off(int64_t n, int64_t k, int64_t K) {
    return ((n >> 4) * (K >> 6) + (k >> 6)) * 512 + ((((k & 31) >> 3) << 4) + (n & 15)) * 8 + ((k & 63) >> 5) * 4 + ((k & 7) >> 1);
}
__host__ __device__ __forceinline__ int64_t mx4_scale_off(int64_t n, int64_t kb, int64_t K) {
    return ((n >> 4) * (K >> 6) + (kb >> 1)) * 32 + (n & 15) * 2 + (kb & 1);
}
constexpr int W4_EXP_MIN = W8_EXP_MIN;      // floor of the block exponents: the scale byte e + 127 is never 0 (nor 255)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// 16 e2m1 codes (one lane's 8 bytes of an MXFP4 code block) and the two scale bytes of (row, chunk) in the low 16 bits of s2 ->
// the two B operands of the chunk: v_cvt_scalef32_pk_{f16,bf16}_fp4 multiplies by the fp32 whose exponent byte is the scale and
// whose mantissa is zero, so the results ARE the dequantised weights (normal numbers of the operand type or zero, by the
// quantiser's flush rule)
__device__ __forceinline__ void mx4x16_to_h8(u32x2 q, uint32_t s2, h8 &lo, h8 &hi) {
    const float s0 = __builtin_bit_cast(float, (s2 & 0xffu) << 23), s1 = __builtin_bit_cast(float, (s2 & 0xff00u) << 15);
#ifdef OPUS_BF16
#define OPUS_CVT_FP4(w, sc, sel) __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((w), (sc), sel)
#else
#define OPUS_CVT_FP4(w, sc, sel) __builtin_amdgcn_cvt_scalef32_pk_f16_fp4((w), (sc), sel)
#endif
    const h2 a0 = OPUS_CVT_FP4(q[0], s0, 0), a1 = OPUS_CVT_FP4(q[0], s0, 1), a2 = OPUS_CVT_FP4(q[0], s0, 2), a3 = OPUS_CVT_FP4(q[0], s0, 3);
    const h2 b0 = OPUS_CVT_FP4(q[1], s1, 0), b1 = OPUS_CVT_FP4(q[1], s1, 1), b2 = OPUS_CVT_FP4(q[1], s1, 2), b3 = OPUS_CVT_FP4(q[1], s1, 3);
#undef OPUS_CVT_FP4
    lo = h8{a0[0], a0[1], a1[0], a1[1], a2[0], a2[1], a3[0], a3[1]};
    hi = h8{b0[0], b0[1], b1[0], b1[1], b2[0], b2[1], b3[0], b3[1]};
}
// One lane's share of an MXFP4 16-row x 64-k weight block in registers, the lane's base pointers into the code and scale panels,
// the load of chunk c and the conversion to the two B operands (gemm_skinny_kernel's W4 form)
struct mx4reg { u32x2 q; uint32_t s; };
struct mx4ptr { const uint8_t *q, *s; };
__device__ __forceinline__ mx4reg q_load(mx4ptr qp, int64_t c) {
    return mx4reg{__builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(qp.q + c * 512)),
                  __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(qp.s + c * 32))};
}
__device__ __forceinline__ void q_to_h8(mx4reg q, h8 &lo, h8 &hi) { mx4x16_to_h8(q.q, q.s, lo, hi); }
// quant.hip: q4 (code panels, N K / 2 bytes), s4 (scale panels, N K / 32 bytes), dq (operand type, row-major [N, K]; may be null or
// src) from row-major src [N, K]; *bad (device, zeroed by the caller) is set when a weight is not finite
hipError_t launch_quantize_mxfp4(const half_t *src, int64_t N, int64_t K, uint8_t *q4, uint8_t *s4, half_t *dq, int *bad, hipStream_t s);

constexpr int HANDOFF_WORDS = 1024, HANDOFF_ERR = 1023;
constexpr int HANDOFF_SPIN_LIMIT = 1 << 19;   // polls (s_sleep(4) + one L2 round trip each: >= 0.3 s) before a waiter gives up

// Which quantised form of a weight matrix, if any, and where it lives (device pointers).  WQ_FP8: codes = fp8_tiled_off panels,
// scales = one int8 exponent per row.  WQ_MXFP4: codes = mx4_code_off panels, scales = mx4_scale_off panels of e8m0 bytes.
// fmt != WQ_NONE means both pointers are set.  Plain data on purpose: the kernels cast `scales` where they read it - a member
// function called on the kernel argument (its `this`) cost gemm_skinny_kernel's LDS-staged FP8 instantiations 4 VGPRs.
enum WeightQuant { WQ_NONE = 0, WQ_FP8 = 1, WQ_MXFP4 = 2, WQ_COUNT };
struct QuantW {
    int fmt = WQ_NONE;
    const uint8_t *codes = nullptr;
    const void *scales = nullptr;
};

struct GemmParams {
    const half_t *A;        // fp16 activations [M,K] (row-major, lda), or
    const float *Af;        // fp32 residual stream [M,K]: fused RMSNorm (skinny kernel only), else nullptr
    float norm_eps;
    int64_t lda;
    const half_t *W;        // panel-tiled [N,K] (see gemm.hip)
    int M, N, K;
    const float *bias;      // [N] or nullptr
    const float *residual;  // fp32 [M,Nout] or nullptr (may alias C when C is fp32)
    int64_t ldr;
    void *C;
    int64_t ldc;
    int out_f32;            // 1: C is fp32, 0: fp16
    int epi;
    float *ws;              // split-K workspace (fp32 partial slabs) or nullptr
    int64_t ws_bytes;
    // Row-scale fusion (RMSNorm between a split-K GEMM and the wide kernel that consumes its output):
    //  producer side - the flat split-K reduce (EPI_NONE, fp32 output, N % 256 == 0) also writes the row as fp16 to xh_out
    //  and the sum of squares of each 256-column block to ssq_out[m * N/256 + j], then sets *fused_done;
    //  consumer side - gemm_wide_kernel multiplies row m of its result by rsqrt(sum_j row_ssq[m * row_nblk + j] / K + norm_eps).
    //  The blocks are 256 columns wide when a split-K reduce (or the embedding kernel) produced them and 16 columns wide when
    //  gemm_stream_kernel did: *nblk_out (HOST) receives the number of blocks per row the producer wrote (at most ssq_cap floats
    //  in all), the consumer gets it back as row_nblk.
    half_t *xh_out;
    float *ssq_out;
    int *fused_done;
    const float *row_ssq;
    int row_nblk;
    int64_t ssq_cap = 0;
    int *nblk_out = nullptr;
    // slab_only: when the launch splits K over workgroups, leave the raw fp32 k-part slabs in ws ([ks][M][N], no epilogue) and
    // report their number in *ks_out instead of launching the reduce - the consumer (attn_decode_kernel) sums them, applies the
    // row scale and the bias itself; *ks_out = 1 means the kernel wrote the finished output as usual.
    int slab_only = 0;
    int *ks_out = nullptr;
    int force_wide = 0;     // route a narrow output (N < 16384) through gemm_wide_kernel + k-parts
    // ESM rotary fused into the epilogue of the QKV projection (gemm_pp_kernel, head_dim 64, fp16 output): columns
    // < rope_cols are rotated in heads of 64 - pairs (d, d + 32), angle of position (row % rope_T) from the [T][32][2]
    // (cos, sin) table - after the usual rounding to fp16, columns < rope_qcols being scaled by rope_qscale first: the same
    // arithmetic as esm_rope_kernel on the stored projection.  *rope_done = 1 when the launch applied it.
    const float *rope_cs = nullptr;
    const int32_t *rope_pos = nullptr;      // token-packed batches: position of every row (instead of row % rope_T)
    int rope_T = 0, rope_cols = 0, rope_qcols = 0;
    float rope_qscale = 1.0f;
    int *rope_done = nullptr;
    // Fragment-ordered ("tiled") activation matrices of the batched decode step (gemm_stream.hip, "Activation layout"):
    // element (row, k) of an [rows, K] matrix at tiled_off(row, k, K).  a_tiled: A is stored that way (gemm_stream_kernel only);
    // xh_tiled / c_tiled: write xh_out / the fp16 output C that way (for a consumer that will read it with a_tiled).
    int a_tiled = 0, xh_tiled = 0, c_tiled = 0;
    // gemm_stream_kernel with k-parts and a finished output: ticket counters (one int per column group, all zero between
    // launches) of the in-launch combine; nullptr: slabs + a split-K reduce launch.  HANDOFF_WORDS ints: [0, 512) tickets of
    // gemm_stream_kernel, [512, HANDOFF_ERR) (ticket, flag) pairs of gemm_pp_kernel's two-part tail tiles, [HANDOFF_ERR] the
    // error word a hand-off sets when its bounded wait runs out (the host reads it at its next synchronisation: OPUS_EHIP).
    // Everything below HANDOFF_ERR is zeroed at the head of every encode / prefill / decode step.
    int *combine_cnt = nullptr;
    // LayerNorm fused around the big tiled GEMM (gemm_pp_kernel; the encoder's pre-LN blocks).  With the norm
    // weight folded into the consumer's weight W' = W diag(gamma) and beta into its bias c2 = W beta + b,
    //   LN(x) W^T + b  =  rstd (x W'^T - mu s) + c2,   s[n] = sum_k W'[n][k]:
    //  producer side (fp32 output + residual, EPI_NONE, N % 256 == 0): the epilogue also writes fp16(x) to xh_out (row-major)
    //   and, per row and 64-column slab, (sum x, sum x^2) to ln_part[(m * N/64 + slab) * 2]; sets *ln_done;
    //  consumer side (fp16 output, EPI_NONE / GELU): A is fp16(x) as it stands, ln_stat[m] = (mu, rstd), ln_colsum = s,
    //   bias = c2; the epilogue applies the affine form above before the activation / the fused rotary.
    //  RMSNorm (the decoder prefill) is the same with mu = 0: ln_colsum = nullptr, any epilogue incl. the gate / up pair.
    float *ln_part = nullptr;
    int *ln_done = nullptr;
    const float *ln_stat = nullptr;
    const float *ln_colsum = nullptr;
    int pp_gm = 8;                // gemm_pp_kernel: tile rows per rasterisation group (8 = an 8 x 4 tile patch per XCD)
    int stagger = 0;              // gemm_pp_kernel: late start of half of the first round, in units of ~4 us (see the kernel)
    int no_rot = 0;               // A/B aid (OPUS_NO_KROT): weight-streaming kernels walk k from chunk 0 in every workgroup
    long long *trace = nullptr;   // tuning aid (OPUS_PP_TRACE): gemm_pp_kernel writes 4 wall-clock stamps per workgroup
    // launch_pp reports what it launched in pp_plan[0 .. PP_PLAN_WORDS) (HOST; nullptr: no report, nothing else changes):
    // [0] tiles of whole K, [1] tail tiles cut into k-parts, [2] k-parts per tail tile (1: no tail split), [3] how the parts are
    // combined (PP_TAIL_NONE / PP_TAIL_PAIR: inside the launch / PP_TAIL_REDUCE: pp_tail_reduce_kernel), [4] 1 = the rotary ran
    // in the epilogue.  A GEMM that another kernel takes leaves the words as they were.
    int *pp_plan = nullptr;
    // every launcher reports what it launched in plan[0 .. GEMM_PLAN_WORDS) (HOST; nullptr: no report, nothing else changes):
    // [0] kernel class (KC_*), [1] row-tile template argument (MT; TM of the ring kernel; 0: the kernel has none), [2] / [3] TN / NS
    // of the ring kernel (else 0), [4] the skinny kernel's ALDS flag (else 0), [5] the stream kernel's P (else 0), [6] k-parts over
    // workgroups (gemm_pp_kernel: per tail tile; 1: K is not cut), [7] how the k-parts become the output (GemmCombine)
    int *plan = nullptr;
    // Quantised form of W (the same values as W): a kernel that has an instantiation for wq.fmt streams it instead of W and sets
    // *ran_wq (HOST) = wq.fmt; every other kernel reads W as ever and leaves *ran_wq alone
    QuantW wq;
    int *ran_wq = nullptr;
};
constexpr int PP_PLAN_WORDS = 5;
enum PpTail { PP_TAIL_NONE = 0, PP_TAIL_PAIR = 1, PP_TAIL_REDUCE = 2 };
constexpr int GEMM_PLAN_WORDS = 8;
// GC_NONE: one k-part; GC_REDUCE / GC_REDUCE4: splitk_reduce_kernel / splitk_reduce4_kernel behind the launch; GC_IN_LAUNCH: the
// workgroup of gemm_stream_kernel that arrives last; GC_PP_PAIR / GC_PP_REDUCE: gemm_pp_kernel's pair hand-off / pp_tail_reduce_kernel;
// GC_SLABS: nobody here - the raw slabs are the result (GemmParams::slab_only)
enum GemmCombine { GC_NONE = 0, GC_REDUCE = 1, GC_REDUCE4 = 2, GC_IN_LAUNCH = 3, GC_PP_PAIR = 4, GC_PP_REDUCE = 5, GC_SLABS = 6 };
inline void gemm_plan_set(const GemmParams &p, int klass, int mt, int tn, int ns, int alds, int P, int ks, int combine) {
    if (!p.plan) return;
    const int v[GEMM_PLAN_WORDS] = {klass, mt, tn, ns, alds, P, ks, combine};
    for (int i = 0; i < GEMM_PLAN_WORDS; ++i) p.plan[i] = v[i];
}

// Flash-style attention over strided Q/K/V (fp16).  Q(b,h,t,:) = Q + b*q_sb + t*q_st + h*HD etc.;
// kv head of q head h is h / group.  Key j of batch row b is visible to query i iff
// kstart[b] <= j < kend[b] and (!causal || j <= i).  O is [B, T, heads*HD] row-major fp16.
struct AttnParams {
    const half_t *Q, *K, *V;
    int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st;
    half_t *O;
    int64_t o_sb, o_st;
    const int32_t *kstart;  // [B] or nullptr (= 0)
    const int32_t *kend;    // [B] or nullptr (= T)
    int B, T, heads, group, head_dim, causal;
    float scale;
    // Token-packed ("varlen") batches: cu[B + 1] row offsets into Q / K / V / O, whose rows are the batch rows' tokens back to
    // back with no padding (q_sb / k_sb / v_sb / o_sb unused).  Row b has cu[b + 1] - cu[b] tokens, all of them visible keys
    // (kstart / kend unused); T = the longest row (sizes the grid).
    const int32_t *cu = nullptr;
    int q_trim = 0;         // token-packed only: 1 = the first and the last token of every row are keys but not queries (last ESM-2 layer)
};

hipError_t launch_gemm(const GemmParams &p, hipStream_t s, int *klass);
// gemm_stream.hip: one-launch weight streaming for narrow outputs at 5..64 rows (K cut over the waves of a workgroup)
hipError_t launch_splitk_reduce(const GemmParams &p, int ks, hipStream_t s);   // gemm.hip: sums the k-part slabs in p.ws, applies the epilogue
bool gemm_stream_ok(const GemmParams &p);
bool gemm_stream_would(int M, int N, int K, int slab_only, int a_tiled, int row_scale, int64_t ws_bytes);
hipError_t launch_gemm_stream(const GemmParams &p, hipStream_t s);
// Run-time tuning knobs (A/B aids; opus_debug_knob sets them, environment variables give the defaults)
struct Knobs {
    int no_stream = 0;      // 1: narrow decode GEMMs take the round-2 kernels (gemm_wide / gemm_ring / gemm_mid + reduce)
    int no_ln_fusion = 0;   // 1: stand-alone normalisation kernels instead of the norms fused around gemm_pp_kernel
    int debug_a_tiled = 0;  // 1: opus_debug_gemm takes A in fragment order (GemmParams::a_tiled)
    int pp_gm = 8;          // tile-rows per group of the gemm_pp / gemm_ring rasterisation
    int enc_full_last_layer = 0;   // 1: the packed encoder's last layer computes the <cls> / <eos> rows too (AttnParams::q_trim off)
    int misc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // scratch knobs for experiments
};
extern Knobs g_knobs;
// rstd[r] = rsqrt(sum_j ssq[r * nblk + j] / K + eps) for rows r < rows, computed by the whole workgroup (NWAVES waves) into
// LDS `out`: every load of a wave's rows is requested before the first sum (one round trip, not nblk / 4)
template <int NWAVES, int ROWS>
__device__ __forceinline__ void block_row_rstd(const float *__restrict__ ssq, int M, int nblk, float inv_k, float eps, float *out,
                                               int wave, int lane) {
    constexpr int RW = (ROWS + NWAVES - 1) / NWAVES;
    float part[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) part[r] = 0.f;
    for (int j0 = 0; j0 < nblk; j0 += 256) {
        float t[RW][4];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            int row = wave + NWAVES * r;
            row = row < M ? row : M - 1;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 64 * u + lane;
                t[r][u] = ssq[(int64_t)row * nblk + (j < nblk ? j : nblk - 1)];
                t[r][u] = j < nblk ? t[r][u] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) part[r] += (t[r][0] + t[r][1]) + (t[r][2] + t[r][3]);
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float q = part[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const int row = wave + NWAVES * r;
        if (lane == 0 && row < ROWS) out[row] = rsqrtf(q * inv_k + eps);
    }
}
bool gemm_goes_wide(int M, int N);
bool gemm_goes_pp(int M, int N);     // would launch_gemm route an fp16-A GEMM of this shape to gemm_pp_kernel (the big tiled kernel)?   // would launch_gemm route an fp16-A GEMM of this shape to gemm_wide_kernel?
hipError_t launch_attn_prefill(const AttnParams &p, hipStream_t s);
int attn_prefill_query_tiles(const AttnParams &p);   // 16-query tiles per wave (1 / 2) that launch_attn_prefill takes for p (HOST)
// attn_prefix.hip: attention of continuation rows over a cached prefix + their own positions (opus_llama_score_continuations).
// Continuation row r has n positions at rows r n .. r n + n - 1 of qkv ([rows][(nh + 2 nkv) hd], q and k rotated); the rows that
// belong to prefix row p are list[off[p] .. off[p + 1]).  Keys: cache slots kstart[p] .. Tp - 1 of row p ([P][nkv][slot][hd] at
// kc / vc with strides cache_sb / cache_sh), then the row's own positions 0 .. t.  blocks: (p, first stacked query) per workgroup
// (attn_prefix_blocks).  out: [rows][nh hd].
struct AttnPrefixParams {
    const half_t *kc, *vc;
    int64_t cache_sb, cache_sh;
    const int32_t *kstart;
    int Tp;
    const half_t *qkv;
    int n;
    const int32_t *list, *off, *blocks;
    half_t *out;
    int nh, nkv, hd;
    float scale;
    const int32_t *par = nullptr;   // tree form only (selects it): parent row of every row of the pass (-1: a child of the root)
};
// workgroup table of launch_attn_prefix for the row lists off[0 .. P] (blocks = nullptr: count only); returns the block count
int attn_prefix_blocks(const int32_t *off, int P, int G, int n, int32_t *blocks);
int attn_prefix_max_blocks(int R, int P, int G, int n);   // an upper bound of that count for R rows over P prefix rows
// par set selects the tree form (opus_llama_score_tree): n must be 1 (one new position per row: a trie node) and row r attends to
// the cache slots of its prefix row, then to r, par[r], par[par[r]], ... (rows of this pass, the chain ends at -1).
hipError_t launch_attn_prefix(const AttnPrefixParams &p, int nblocks, hipStream_t s);

// kv_place.hip: the bandwidth kernels of detached prefixes (opus_llama_prefix_export, opus_llama_prefill_behind).  A snapshot holds
// K (or V) of `rows` cache rows as [layers][rows][nkv][T][hd], slot 0 first; the live cache is kc / vc with strides cache_sl /
// cache_sb / cache_sh (halfs).  hd is a multiple of 8 and every base 16-byte aligned: the copies move 16 bytes per lane.
// export: snapshot <- rows 0 .. R - 1, slots 0 .. T - 1 of every layer of the cache (one launch, K and V)
hipError_t launch_kv_export(const half_t *kc, const half_t *vc, int64_t cache_sl, int64_t cache_sb, int64_t cache_sh, int layers, int R,
                            int nkv, int T, int hd, half_t *snap_k, half_t *snap_v, hipStream_t s);
// export rows (the inverse of place, for the ragged cache a decode loop leaves): the window kstart[r] .. kstart[r] + Tp - nks[r] - 1
// of cache row r -> slots nks[r] .. Tp - 1 of snapshot row r, zeros below nks[r]; all layers, K and V, one launch.  Every row then
// ends at the snapshot's last slot, as launch_kv_place expects.  The caller has checked every window against the cache's slots.
struct KvExportRowsParams {
    const half_t *kc, *vc;
    int64_t cache_sl, cache_sb, cache_sh;
    const int32_t *kstart;          // [R] device: first slot of every row's window in the cache
    const int32_t *nks;             // [R] device: first visible slot of every snapshot row (Tp - window length)
    int R, Tp;
    half_t *snap_k, *snap_v;
    int layers, nkv, hd;
};
hipError_t launch_kv_export_rows(const KvExportRowsParams &p, hipStream_t s);
// place: the visible slots kstart[p] .. Tp - 1 of snapshot row p -> every decode row r of list[off[p] .. off[p + 1]) at slots
// new_kstart[r] .. new_kstart[r] + Tp - kstart[p] - 1, all layers, K and V, one launch; each 16-byte piece is read once and stored
// to all the rows of its prefix row.  Nothing else of the cache is written.
struct KvPlaceParams {
    const half_t *snap_k, *snap_v;
    const int32_t *kstart;          // [P] device: first visible slot of every snapshot row
    int P, Tp;
    half_t *kc, *vc;
    int64_t cache_sl, cache_sb, cache_sh;
    const int32_t *list, *off;      // decode rows grouped by prefix row (PrefixTables)
    const int32_t *new_kstart;      // [R] device: first visible slot of every decode row
    int layers, nkv, hd;
};
hipError_t launch_kv_place(const KvPlaceParams &p, hipStream_t s);
// append (one layer): rotated K and the V of the suffix positions t < lens[r] of the R rows in qkv ([R n][(nh + 2 nkv) hd]) -> cache
// row r at slot Tp + (n - lens[r]) + t
hipError_t launch_kv_append(const half_t *qkv, const int32_t *lens, int R, int n, int nh, int nkv, int hd, int Tp, half_t *kc, half_t *vc,
                            int64_t cache_sb, int64_t cache_sh, hipStream_t s);

// stream.hip: continuous batching (opus_stream_*).  start [B]: the step a row's occupant began at; poll [B + 1]: the rows' end steps
// (-1: not done) and, in poll[B], the count of rows not done - what the host copies out behind every step.
// finish (behind the step kernel of step t = step[0]): a row whose budget is used up (t + 1 - start[r] >= max_new) is marked
// finished; the first step at which a row is done goes to poll[r]
hipError_t launch_stream_finish(const int32_t *step, const int32_t *start, int32_t *fin, int32_t *poll, int B, int max_new, hipStream_t s);
// refill (step boundary t): listed row i = decode row rows[i] takes row src[i] of logits_in [*, V], kstart nks[rows[i]], start t,
// cleared fin / poll words and -1 in id columns t - 8 .. t - 1 (ids [B, S])
hipError_t launch_stream_refill(const int32_t *rows, const int32_t *src, const int32_t *nks, int n, const float *logits_in, float *logits,
                                int V, int32_t *kstart, int32_t *start, int32_t *fin, int32_t *poll, int32_t *ids, int S, int t,
                                hipStream_t s);
hipError_t launch_stream_reset(int32_t *start, int32_t *poll, int B, hipStream_t s);

// contact.hip: ESM-2 contact maps (opus_esm2_contacts_packed).  One layer's accumulation over token-packed proteins cu[B + 1]
// (rows <cls> residues <eos>): Q / K rows of stride ld (head h at column h hd; q scaled and both rotated as the attention takes
// them); A[sum n_b^2] (+)= sum_h w[h] P_h over the interior positions, rows[(cu[b] - 2 b + i) vld + c0 + h] = interior row sums
// of P_h, part = the column-sum partials that launch_esm_contact_colsum reduces into the same layout (add: += instead of =).
struct ContactParams {
    const half_t *Q, *K;
    int64_t ld;
    const int32_t *cu;
    int B, heads;
    const float *w;
    float *A;
    int accumulate;
    float *rows;
    int64_t vld;
    int c0;
    float *part;
};
size_t contact_accum_lds(int heads);
hipError_t launch_esm_contact_accum(const ContactParams &p, int head_dim, int max_n, hipStream_t s);   // max_n: longest n_b
hipError_t launch_esm_contact_colsum(const float *part, const int32_t *cu, int B, int heads, int max_n, float *vec, int64_t vld, int c0,
                                     int add, hipStream_t s);
// sw[b][c] = w[c] / sum_i vec[i][c] over protein b's rows; then out = sigmoid(bias + A + A^T - sum_c sw_c a_c a_c^T) (vec [.][C] = a)
hipError_t launch_esm_contact_scale(const float *vec, const int32_t *cu, int B, int C, const float *w, float *sw, hipStream_t s);
hipError_t launch_esm_contact_finish(const float *A, const float *vec, const float *sw, const int32_t *cu, int B, int C, int max_n,
                                     const float *bias, float *out, hipStream_t s);

// norm.hip
// mlm.hip: ESM-2 masked-LM head (opus_esm2_lm_head).  launch_mlm_gather: rows idx[0 .. R) (null: 0 .. R - 1) of the fp32 states
// src [src_rows, D] -> operand rows dst [Mg, D], rows R .. Mg - 1 zero, an index out of range a NaN row.  launch_mlm_head:
// out[R, V] = LN(y) We^T + bias (We row-major [V, D], V <= 64), log-softmax over the V columns on request.
hipError_t launch_mlm_gather(const float *src, int64_t src_rows, const int32_t *idx, int R, int Mg, int D, half_t *dst, hipStream_t s);
hipError_t launch_mlm_head(const half_t *y, const float *lnw, const float *lnb, float eps, const half_t *We, const float *bias,
                           int64_t R, int D, int V, int log_softmax, float *out, hipStream_t s);
hipError_t launch_layernorm(const float *x, const float *w, const float *b, float eps, int64_t rows, int D,
                            half_t *out_h, float *out_f, hipStream_t s);   // (w == b == nullptr: (x - mu) rstd, no affine part)
// (mu, rstd) per row from the per-slab (sum x, sum x^2) partials the LayerNorm-producing GEMM epilogue left (GemmParams::ln_part)
// (rms != 0: RMSNorm - (0, rsqrt(mean x^2 + eps)))
hipError_t launch_ln_finalize(const float *part, int64_t rows, int nslab, int D, float eps, int rms, float *stat, hipStream_t s);
hipError_t launch_rmsnorm(const float *x, const float *w, float eps, int64_t rows, int D, half_t *out,
                          hipStream_t s);
hipError_t launch_l2norm(const float *x, int64_t rows, int D, half_t *out, hipStream_t s);
hipError_t launch_f2h(const float *x, int64_t n, half_t *out, hipStream_t s);
hipError_t launch_masked_mean(const float *h, const int32_t *lens, int B, int T, int D, float *out,
                              hipStream_t s);
// token-packed forms (cu[B + 1] row offsets; Tmax = the longest row): embedding, pooling, and the row -> position table
hipError_t launch_masked_mean_packed(const float *h, const int32_t *cu, int B, int D, float *out, hipStream_t s);
hipError_t launch_esm_embed_packed(const int32_t *tok, const half_t *emb, const int32_t *cu, int B, int Tmax, int D, float *x,
                                   int32_t *pos, hipStream_t s);

// elementwise.hip
hipError_t launch_esm_embed(const int32_t *tok, const half_t *emb, int B, int T, int D, float *x, hipStream_t s);
hipError_t launch_esm_rope(half_t *qkv, const float *cs, int B, int T, int heads, int hd, float qscale,
                           hipStream_t s, const int32_t *pos = nullptr);   // pos: per-row positions (packed batches; B * T rows)
hipError_t launch_dec_rope_cache(half_t *qkv, const float *cs, const int32_t *kstart, int B, int T, int nh,
                                 int nkv, int hd, half_t *kc, half_t *vc, int64_t cache_sb, int64_t cache_sh,
                                 hipStream_t s, int nret = 1);   // nret > 1: prompt b's K / V to the cache rows b nret + j, j < nret
// dst[b nret + j] = src[b] (fp32 rows of width V, src != dst) and kstart[0 .. B) -> kstart[b nret + j] in place (staged in LDS)
hipError_t launch_row_fanout(const float *src, float *dst, int V, int B, int nret, int32_t *kstart, hipStream_t s);
hipError_t launch_h2f(const half_t *in, float *out, int64_t n, hipStream_t s);
// x[b,:] = fp32(emb[tok[b]]); optionally also the fp16 copy xh and the per-256-column sums of squares ssq[b][H/256] (the
// producer side of the row-scale RMSNorm fusion, GemmParams::row_ssq)
// ... and (cs != nullptr) the rotary rows of this step: cs_row[b][d] = cs[T0 + *step - kstart[b]][d], d < half (float2 each)
hipError_t launch_embed_tokens(const int32_t *tok, const half_t *emb, int B, int H, int V, float *x, half_t *xh, float *ssq,
                               int xh_tiled, const float *cs, const int32_t *kstart, const int32_t *step, int T0, int half,
                               float *cs_row, int *cnt, int ncnt, hipStream_t s);
hipError_t launch_add_pos(float *x, const half_t *pos, const int32_t *kstart, const int32_t *step, int t0, int B, int Tq,
                          int H, int max_idx, hipStream_t s);
hipError_t launch_take_last(const float *x, int B, int T, int H, float *out, hipStream_t s);
// score.hip: out[r] = x[rows[r]] (fp32 rows of width H; an index outside [0, n_src) gives a zero row)
hipError_t launch_gather_rows(const float *x, const int32_t *rows, int R, int64_t n_src, int H, float *out, hipStream_t s);
// out[r] = rows[r] >= 0 ? x[rows[r]] : y[-rows[r] - 1] (two sources: continuation rows and the prefix's last rows)
hipError_t launch_gather_rows2(const float *x, int64_t n_x, const float *y, int64_t n_y, const int32_t *rows, int R, int H, float *out,
                               hipStream_t s);
// score.hip: per row r of logits [R, V] (row stride ld): lse[r] = logsumexp, logprob[r] = l[targets[r]] - lse[r] (fp32;
// target < 0: 0, target >= V: NaN; lse may be null)
hipError_t launch_xent(const half_t *logits, int64_t ld, int R, int V, const int32_t *targets, float *logprob, float *lse,
                       hipStream_t s);
// score.hip: trie scoring behind launch_xent's lse over the n logits rows of a chunk [n, V].  Edge e (row erow[e] - row0 of the
// chunk, token etok[e]) writes node_lp[eslot[e]] = l[row][tok] - lse[row]; stop entry k (row srow[k] - row0, id set sset[k] =
// ids[soff[set] .. soff[set + 1])) writes stop_lp[sslot[k]] = log sum_ids exp(l[row][id] - lse[row]), ids added in list order.
hipError_t launch_tree_edges(const half_t *logits, int64_t ld, const float *lse, int row0, const int32_t *erow, const int32_t *etok,
                             const int32_t *eslot, int n_edges, float *node_lp, const int32_t *srow, const int32_t *sset,
                             const int32_t *sslot, int n_stops, const int32_t *ids, const int32_t *soff, float *stop_lp, hipStream_t s);
// score.hip: member_lp[p, m] = sum of node_lp[p, v] over the path of member node mnode[trie[p], m] in root-to-leaf order (fp32;
// -inf where mnode < 0).  par / depth [tries, ld_nodes] describe each distinct trie, node_lp [P, ld_nodes], mnode [tries, M].
hipError_t launch_tree_path_sums(const float *node_lp, const int32_t *trie, const int32_t *par, const int32_t *depth,
                                 const int32_t *mnode, int P, int M, int ld_nodes, float *member_lp, hipStream_t s);
hipError_t launch_relu_h(half_t *x, int64_t n, hipStream_t s);
hipError_t launch_fill_synth(void *dst, int dtype, int64_t rows, int64_t cols, uint64_t seed, float std,
                             float mean, int64_t rb, int64_t rs, int64_t ro, int tiled, uint64_t fold_seed,
                             float fold_std, float fold_mean, hipStream_t s);
hipError_t launch_argmax_partial(const float *logits, int B, int V, float *pval, int32_t *pidx, hipStream_t s);
hipError_t launch_tile_weight(const half_t *src, half_t *dst, int64_t N, int64_t K, hipStream_t s);
hipError_t launch_lora_merge(half_t *W, const half_t *A, const half_t *B, float scale, int64_t out_f,
                             int64_t in_f, int r, hipStream_t s);
hipError_t launch_splice_plan(const int64_t *ids, const uint8_t *mask, int B, int Tt, int n_tok, int max_len,
                              int V, int32_t *plan, hipStream_t s);
hipError_t launch_splice_fill(const int64_t *ids, const uint8_t *mask, int B, int Tt, const half_t *prot,
                              int n_tok, int H, int V, const half_t *emb, const int32_t *plan, int Tout,
                              int left_pad, half_t *out, uint8_t *mask_out, int32_t *pos_out, hipStream_t s);
// (thr_out != nullptr: no draw; the rows' keep thresholds on p = exp(l / T - max / T) are written there - beam-sample.
//  psum != nullptr: the first pass is argmax_lse_partial (part sums for the log-sum-exp); thr_keep != nullptr: the draw also
//  exports its keep thresholds there)
hipError_t launch_sample_select(const float *logits, int B, int V, float temperature, float top_p, int top_k, const uint64_t *seed,
                                const int32_t *step, float *pmax, int32_t *pidx, float *cand_p, int32_t *cand_i,
                                int32_t *cand_n, float *zpart, float *spart, int32_t *chosen, float *thr_out, float *psum,
                                float *thr_keep, hipStream_t s);
// The sampling warpers behind top-k / top-p (opus_set_sampling_warpers), read by the captured step from device memory.  Off: 0, 1, 0, 0.
struct SamplingWarpers {
    float min_p, typical_p, epsilon, eta;
};
// Behind launch_sample_select(chosen = nullptr, thr_out = thr_lo): the warpers narrow the kept set to the band thr_lo[b] < p <=
// thr_hi[b] (both written back), then the draw over it into chosen.
hipError_t launch_sample_warp_draw(int B, int V, const SamplingWarpers *warp, const uint64_t *seed, const int32_t *step,
                                   const float *cand_p, const int32_t *cand_i, const int32_t *cand_n, int32_t *chosen, float *thr_lo,
                                   float *thr_hi, hipStream_t s);
constexpr int APART = 64;     // parts a logits row is cut into by argmax_partial / sample_stage1 (pmax[row * APART + part])
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
hipError_t launch_argmax_step(const float *pval, const int32_t *pidx, const int32_t *chosen, int B, const int32_t *eos, int n_eos, int pad_id,
                              int32_t *finished, int32_t *out_ids, int max_new, const int32_t *step,
                              int32_t *next_tok, int32_t *n_unfinished, const int32_t *stop, int n_stop, hipStream_t s);
hipError_t launch_step_advance(int32_t *step, hipStream_t s);
// generate()'s optional outputs, read by the captured step from device memory (opus_generate_scored writes the descriptor before
// its loop): token_lp [B, max_new], scores / logits [max_new, B, V], fp32, rows and steps indexed by the device step word; null = off.
// top_lp / top_ids [B, max_new, top_k] (opus_set_gen_top_logprobs): the k likeliest tokens of the raw row and their log-probabilities
struct GenOutDesc {
    float *token_lp;
    float *scores;
    float *logits;
    float *top_lp;
    int32_t *top_ids;
    int32_t top_k;
    int32_t pad_;
};
// topk.hip: the k <= TOPK_MAX likeliest entries of each of R logits rows (value descending, then index ascending) and their
// log-probabilities l[id] - lse, in two launches: the k best of every one of the row's APART parts into cand [R, APART, TOPK_MAX]
// (64-bit keys), then a wave per row merges them.  The lse: lse[row], or (lse == nullptr) parts_lse over pval / psum [R, APART] of
// argmax_lse_partial on the same rows.  Where to: desc != nullptr (the captured step) - desc->top_ids / top_lp / top_k, read on the
// device; else ids / lp / k.  step != nullptr: [row, *step, :] of a [R, max_new, k] array, nothing when *step >= max_new; else [row, :].
// finished != nullptr: a row whose word is set gets ids -1 and log-probs 0.
constexpr int TOPK_MAX = 20;
struct TopkArgs {
    uint64_t *cand = nullptr;
    const float *lse = nullptr, *pval = nullptr, *psum = nullptr;
    const int32_t *finished = nullptr, *step = nullptr;
    int max_new = 1;
    const GenOutDesc *desc = nullptr;
    int k = 0;
    int32_t *ids = nullptr;
    float *lp = nullptr;
};
hipError_t launch_topk_f32(const float *logits, int64_t ld, int R, int V, const TopkArgs &a, hipStream_t s);
hipError_t launch_topk_h16(const half_t *logits, int64_t ld, int R, int V, const TopkArgs &a, hipStream_t s);
// lse [R] of rows of either type with a leading dimension (opus_debug_top_logprobs)
hipError_t launch_topk_row_lse(const void *logits, bool f32, int64_t ld, int R, int V, float *lse, hipStream_t s);
// argmax_partial + each part's sum of exp(l - part max) (psum [B, APART])
hipError_t launch_argmax_lse_partial(const float *logits, int B, int V, float *pval, int32_t *pidx, float *psum, hipStream_t s);
// argmax_step + out->token_lp[b, step] = logits[b, tok] - logsumexp(logits[b]) (0 for rows finished before the step)
hipError_t launch_argmax_lse_step(const float *pval, const int32_t *pidx, const float *psum, const int32_t *chosen, int B,
                                  const int32_t *eos, int n_eos, int pad_id, int32_t *finished, int32_t *out_ids, int max_new,
                                  const int32_t *step, int32_t *next_tok, int32_t *n_unfinished, const int32_t *stop, int n_stop,
                                  const float *logits, int V, const GenOutDesc *out, hipStream_t s);
hipError_t launch_argmax_lse_final(const float *pval, const int32_t *pidx, const float *psum, int B, int32_t *idx, float *lse,
                                   hipStream_t s);
// argmax_step + out->token_lp[b, step] = raw - lse[b] when logits processors edited the logits in place (opus_ctx::lproc_on):
// lse [B] is the raw rows' log-sum-exp (taken before the processors ran); raw = raw_hist[b, i] at the first history position i that
// holds the chosen token (logits_proc_kernel recorded the raw value there), else logits[b, tok] (a logit no processor touched)
hipError_t launch_argmax_rawlp_step(const float *pval, const int32_t *pidx, const float *lse, const float *raw_hist,
                                    const int32_t *chosen, int B, const int32_t *eos, int n_eos, int pad_id, int32_t *finished,
                                    int32_t *out_ids, int max_new, const int32_t *step, int32_t *next_tok, int32_t *n_unfinished,
                                    const int32_t *stop, int n_stop, const float *logits, int V, const GenOutDesc *out,
                                    hipStream_t s);
// out->scores / out->logits at the step (thr != nullptr: sampling - l / T where the draw kept the token, -inf elsewhere; thr_hi !=
// nullptr: the kept set is the band thr[b] < p <= thr_hi[b] of launch_sample_warp_draw)
hipError_t launch_gen_scores(const float *logits, int B, int V, const GenOutDesc *out, const int32_t *step, int max_new,
                             float temperature, float top_p, const float *pmax, const float *thr, const float *thr_hi, hipStream_t s);
// logits_proc.hip: generate()'s logits processors (opus_set_logits_processors), read by the captured step from device memory.
// Capacities (include/opus_pllm.h): LP_MAX_BAD bad-word entries of at most LP_MAX_BAD_LEN ids, LP_MAX_BAD_IDS ids in all; a
// history of at most LP_MAX_HIST ids.
constexpr int LP_MAX_BAD = 256, LP_MAX_BAD_LEN = 8, LP_MAX_BAD_IDS = 1024, LP_MAX_HIST = 2048;
struct LogitsProcDesc {
    float penalty;                     // repetition_penalty (1: off)
    int32_t ngram;                     // no_repeat_ngram_size (0: off)
    int32_t min_new;                   // EOS ids are -inf while fewer ids have been generated (0: off)
    int32_t n_bad;                     // bad-word entries: entry e = bad_ids[bad_off[e] .. bad_off[e + 1])
    int32_t bad_off[LP_MAX_BAD + 1];
    int32_t bad_ids[LP_MAX_BAD_IDS];
};
// in place on logits [B, V] (row stride V): the history of row b is hist[b * ld + 0 .. *step) (clamped to max_hist <= LP_MAX_HIST);
// raw_hist (optional) [B, ld] receives the raw logit of every history position
hipError_t launch_logits_proc(float *logits, int B, int V, const int32_t *hist, int64_t ld, const int32_t *step, int max_hist,
                              const int32_t *eos, int n_eos, const LogitsProcDesc *desc, float *raw_hist, hipStream_t s);
// constraint.hip: constrained decoding (opus_set_token_constraint).  The automaton's table and the per-row state words live in
// device memory; the captured step reaches them through this descriptor, so another table needs no new graph.
constexpr int TC_MAX_VOCAB = 1 << 18, TC_MAX_END = 64;     // the allowed set is a V-bit map in LDS (32 KB at the cap)
struct TokenConstraintDesc {
    const int32_t *edge_off;           // [n_states + 1] state s owns the edges edge_off[s] .. edge_off[s + 1)
    const int32_t *edge_tok;           // [n_edges] ids, ascending within a state
    const int32_t *edge_next;          // [n_edges] target states
    const uint8_t *completing;         // [n_states] the end ids are allowed too
    const int32_t *end_ids;            // [n_end]
    const int32_t *start;              // [n_start] start state of every row (n_start == 1: shared)
    int32_t *state;                    // [2, state_stride] the rows' states, double-buffered by the parity of the step
    int32_t n_states, n_end, n_start, state_stride;
    int32_t start_div, unused;         // row b starts at start[b / start_div] (the fanned-out generate: one start state per prompt)
};
// in place on logits [B, V] (row stride V): one transition per row on hist[b * ld + *step - 1] (the start state at *step == 0),
// then -inf outside the state's allowed set.  logits == nullptr: the transition only.
hipError_t launch_token_constraint(float *logits, int B, int V, const int32_t *hist, int64_t ld, const int32_t *step, int max_hist,
                                   const TokenConstraintDesc *desc, hipStream_t s);
// guidance.hip (generate(guidance_scale=g)): the parts' maxima and sums of B rows (an order independent of the rows' alignment), from
// them the rows' maximum, log(sum exp(l - max)) and log-sum-exp; rows cond[b] = g (lsm(cond[b]) - lsm(uncond[b])) + lsm(uncond[b]), lsm(x) = (x - max) - log, in place for n pairs of V-float
// rows (any alignment), g one device float, keep (optional) [n, V] the raw conditional rows; and next[P + b] = next[b]
hipError_t launch_guidance_lse_partial(const float *logits, int B, int V, float *pval, float *psum, hipStream_t s);
hipError_t launch_guidance_lse_final(const float *pval, const float *psum, int B, float *rmax, float *rlog, float *rlse, hipStream_t s);
hipError_t launch_guidance_combine(float *cond, const float *uncond, int n, int V, const float *max_c, const float *log_c,
                                   const float *max_u, const float *log_u, const float *g, float *keep, hipStream_t s);
hipError_t launch_guidance_pair_next(int32_t *next, int P, hipStream_t s);
// beam.hip: best M of the K V continuations per batch row (log_softmax + running scores), cache rows of the surviving beams
hipError_t launch_beam_topk(const float *logits, const float *run, int B, int K, int V, int M, float *lse, float *out_s,
                            int32_t *out_i, hipStream_t s);
// beam-sample: M continuations per batch row drawn without replacement from softmax over the K filtered rows' accumulated
// log-probabilities (thr: launch_sample_select's thresholds, pmax: its per-part maxima), in the order drawn
hipError_t launch_beam_sample(const float *logits, const float *run, int B, int K, int V, int M, float temperature, const float *pmax,
                              const float *thr, int min_keep, float *kth_s, int32_t *kth_i, uint64_t seed, int step, float *lse,
                              float *out_s, int32_t *out_i, hipStream_t s);
hipError_t launch_kv_gather_rows(half_t *cache, half_t *tmp, const int32_t *idx, int R, int64_t row_halfs, int nsub, int64_t sub_halfs,
                                 const int32_t *step, int T0, int hd, int back, hipStream_t s);
hipError_t launch_upload_i32(const int32_t *h, int n, int32_t *dst, hipStream_t s);   // host ints -> device through kernel arguments
// trie_search.hip: one level of search_trie()'s beam search per launch, one workgroup per prompt (opus_trie_search_level)
constexpr int TS_MAXK = 16;            // beams per prompt, and pool entries, at most
struct TrieSearchTable {               // opus_set_trie_search: the tries' children in CSR form; state 0 is the dead state
    const int32_t *edge_off;           // [n_states + 1]
    const int32_t *edge_tok;           // [n_edges] ids, ascending within a state
    const int32_t *edge_next;          // [n_edges] child states
    const int32_t *member;             // [n_states] member index of a state that completes a member, -1 otherwise
    const int32_t *stop_set;           // [n_states] the stop id set of the state's trie
    const int32_t *stop_off;           // [n_sets + 1]
    const int32_t *stop_ids;           // [stop_off[n_sets]]
    int32_t n_states, n_edges;
};
struct TrieSearchLevel {               // == struct opus_trie_search_io behind the logits (include/opus_pllm.h)
    const float *logits;               // rows of `ld` floats: row p K + k of beam k (rows_per_prompt == 1: row p, the first level)
    const float *lse;                  // the rows' log-sum-exp
    int64_t ld;
    int32_t K, top, include_stop, rows_per_prompt;
    const int32_t *state_in;           // [P, K] (in and out may be the same memory)
    const float *score_in;             // [P, K] running scores, -inf = dead
    int32_t *tok, *parent, *state_out; // [P, K] next id, parent ROW (p K + k'), next state; dead: a valid id, the own row, 0
    float *score_out;                  // [P, K] descending, -inf = dead
    int32_t *pool_member;              // [P, top] in / out: best first, -1 = empty
    float *pool_lp, *pool_stop;        // [P, top] member log-prob and stop term (0 without include_stop; -inf where empty)
    int32_t *flags;                    // [P, 3] in / out: live, exhaustive; out: some beam changes its row
    float *edge_lp;                    // [P, K] optional: log-prob of the edge each new beam took
    float *beam_stop;                  // [P, K] optional: stop term of each beam as it stood (-inf: none)
};
hipError_t launch_trie_beam_expand(const TrieSearchTable &t, const TrieSearchLevel &a, int P, int32_t *words, hipStream_t s);
hipError_t launch_mask_to_kstart(const uint8_t *mask, int B, int T, int32_t *kstart, hipStream_t s);

// lookup.hip : prompt-lookup decoding - the n-gram draft, the verify pass's input rows, acceptance and commit in lockstep
struct LookupAcceptParams {
    const int32_t *y;           // [R, n] arg-max of every position of the pass
    const int32_t *x;           // [R, ld_x] the tokens fed: column 0 the last committed token, columns 1 .. the draft
    int ld_x;
    const int32_t *draft_len;   // [R] or nullptr (n - 1 for every row)
    int R, n;
    int pre;                    // 1: a verify pass (commit behind the step word, advance it by a + 1); 0: behind a plain step (n = 1)
    int32_t *ids;               // [R, stride] id matrix or nullptr (opus_llama_verify_step: no commit, no end of a row)
    int stride;
    int32_t *fin;               // [R] finished flags or nullptr
    const int32_t *eos, *stop;
    int n_eos, n_stop, pad;
    int32_t *step;              // the step word
    int32_t *next;              // [R] the last committed token of every row or nullptr
    int32_t *n_unf;             // [stride] rows unfinished behind every column or nullptr
    int32_t *words;             // {a, rows unfinished, step word, ids drafted by unfinished rows}
    int32_t *max_len;           // zeroed for the next draft launch, or nullptr
};
hipError_t launch_lookup_draft(const int32_t *hist, int ld_hist, const int32_t *hist_len, const int32_t *ids, int ld_ids,
                               const int32_t *step, int gen_add, const int32_t *fin, int R, int k, int max_ngram, int filler,
                               int32_t *draft, int ld_draft, int32_t *first, int32_t *draft_len, int32_t *max_len, hipStream_t s);
hipError_t launch_lookup_embed(const int32_t *tok, int ld_tok, int R, int n, const half_t *emb, int H, int V, half_t *x, hipStream_t s);
hipError_t launch_lookup_argmax(const float *pval, const int32_t *pidx, int rows, int32_t *out, hipStream_t s);
hipError_t launch_lookup_accept(const LookupAcceptParams &p, hipStream_t s);
int lookup_max_ngram();

// attn_decode.hip : rope(q,k at the new slot) + cache append + single-query attention
struct AttnDecodeParams {
    const half_t *qkv;          // [B][(nh + 2 nkv) hd] fp16 projection output of the new tokens, or nullptr when slabs != nullptr
    // fused split-K reduce of the QKV GEMM: element (b, col) = (sum_k slabs[k * slab_stride + b * ld + col]) * rstd(b) + bias[col],
    // rstd(b) = rsqrt(sum_j row_ssq[b * row_nblk + j] / K + eps) when row_ssq != nullptr (the fused RMSNorm row scale), else 1
    const float *slabs;
    int ks;
    int64_t slab_stride;
    const float *row_ssq;
    int row_nblk;
    float eps;
    int K;
    const float *bias;
    const float *cs_row;        // [B][hd / 2][2] (cos, sin) of each row's position in THIS step (written by the embedding kernel)
    const int32_t *kstart, *step;   // step[0] = the step counter, step[1] = the prompt length T0 (api.cpp reset_step)
    int T0, nh, nkv;                // T0 < 0: read step[1] (a captured decode step then serves any prompt length)
    half_t *kc, *vc;            // this layer's cache
    int64_t cache_sb, cache_sh;
    int ctx_cap;
    float scale;
    half_t *out;                // [B][nh hd]
    int out_tiled = 0;          // write `out` in fragment order (tiled_off) for a GemmParams::a_tiled consumer
    long long *trace = nullptr; // tuning aid (OPUS_ATTN_TRACE): 8 wall-clock stamps per workgroup
};
hipError_t launch_attn_decode(const AttnDecodeParams &p, int B, int hd, hipStream_t s);
int attn_decode_group(int B, int nh, int nkv);   // the GP (query heads per workgroup) launch_attn_decode takes: 1, 2, 4 or 8

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace opus
