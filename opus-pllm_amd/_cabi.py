"""ctypes binding of include/opus_pllm.h (the only way the Python host reaches the HIP kernels).

There is no fallback: if the shared library has not been built, `lib()` raises and every compute
entry point of the package fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from .config import OpusConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
# OPUS_DTYPE=bf16 (read once, before the first call) selects the bf16-operand build of the same sources (csrc/common.h,
# -DOPUS_BF16); default: fp16, the reference's unquantised dtype (model/builder.py:57)
BF16 = os.environ.get("OPUS_DTYPE", "fp16").lower() in ("bf16", "bfloat16")
LIB_PATH = os.environ.get("OPUS_LIB_PATH") or os.path.join(_HERE, "lib", "libopus_pllm_bf16.so" if BF16 else "libopus_pllm.so")   # (OPUS_LIB_PATH: A/B builds)
ABI_VERSION = 10

OPUS_F16, OPUS_F32, OPUS_I32, OPUS_I64, OPUS_U8 = 0, 1, 2, 3, 4      # (OPUS_F16 = the build's 16-bit operand type)
OPUS_F8E4M3, OPUS_I8 = 5, 6                                          # FP8 decoder weights: the panels' codes, the row exponents
OPUS_F4E2M1X2, OPUS_E8M0 = 7, 8                                      # MXFP4 decoder weights: packed e2m1 pairs, the block scales


def operand_dtype():
    """torch dtype of the library's 16-bit operands (weights, activations, KV cache)."""
    import torch
    return torch.bfloat16 if BF16 else torch.float16


class OpusError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libopus_pllm error {code}: {msg}")
        self.code = code


class CConfig(C.Structure):
    """struct opus_config (include/opus_pllm.h); field order == OpusConfig."""
    _fields_ = [
        ("enc_layers", C.c_int32), ("enc_dim", C.c_int32), ("enc_heads", C.c_int32), ("enc_ffn", C.c_int32),
        ("enc_vocab", C.c_int32), ("enc_ln_eps", C.c_float), ("enc_rope_theta", C.c_float),
        ("has_protein_projector", C.c_int32), ("proj_dim", C.c_int32), ("n_prot_tokens", C.c_int32),
        ("switch_depth", C.c_int32),
        ("dec_layers", C.c_int32), ("dec_dim", C.c_int32), ("dec_heads", C.c_int32), ("dec_kv_heads", C.c_int32),
        ("dec_head_dim", C.c_int32), ("dec_ffn", C.c_int32), ("dec_vocab", C.c_int32),
        ("dec_rms_eps", C.c_float), ("dec_rope_theta", C.c_float),
        ("max_batch", C.c_int32), ("max_enc_tokens", C.c_int32), ("max_prompt", C.c_int32),
        ("max_new_tokens", C.c_int32),
        ("dec_arch", C.c_int32), ("dec_qkv_bias", C.c_int32), ("dec_act", C.c_int32), ("dec_max_pos", C.c_int32),
    ]

    @classmethod
    def from_config(cls, cfg: OpusConfig) -> "CConfig":
        return cls(**{name: getattr(cfg, name) for name, _ in cls._fields_})


_P = C.c_void_p


class CPrefixSnap(C.Structure):
    """struct opus_prefix_snap (include/opus_pllm.h): a detached prefix's K / V, its kstart on the device and on the host."""
    _fields_ = [("d_k", _P), ("d_v", _P), ("d_kstart", _P), ("h_kstart", C.POINTER(C.c_int32)), ("P", C.c_int32), ("Tp", C.c_int32)]


_SNAP = C.POINTER(CPrefixSnap)


class CTrieSearchIO(C.Structure):
    """struct opus_trie_search_io (include/opus_pllm.h): one level's device arrays of search_trie()."""
    _fields_ = [("P", C.c_int32), ("K", C.c_int32), ("top", C.c_int32), ("include_stop", C.c_int32),
                ("d_state", _P), ("d_score", _P), ("d_tok", _P), ("d_parent", _P), ("d_pool_member", _P), ("d_pool_lp", _P),
                ("d_pool_stop", _P), ("d_flags", _P), ("d_words", _P), ("d_lse", _P), ("d_edge_lp", _P), ("d_beam_stop", _P)]


_TSIO = C.POINTER(CTrieSearchIO)
_I32P = C.POINTER(C.c_int32)
# name -> (restype, argtypes): every symbol include/opus_pllm.h declares
SIGNATURES = {
    "opus_llama_prefix_bytes": (C.c_int64, [C.POINTER(CConfig), C.c_int32, C.c_int32]),
    "opus_llama_prefix_export": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "opus_llama_prefill_behind": (C.c_int, [_P, _SNAP, _P, C.c_int32, C.c_int32, _I32P, _I32P, _P, C.POINTER(C.c_int64), _P]),
    "opus_llama_prefix_behind": (C.c_int, [_P, _SNAP, _P, C.c_int32, C.c_int32, _I32P, _I32P, _P, _P, C.POINTER(C.c_int64), _P]),
    "opus_llama_prefix_export_rows": (C.c_int, [_P, C.c_int32, _I32P, C.c_int32, _P, _P, _P, _P]),
    "opus_generate_scored_behind": (C.c_int, [_P, _SNAP, _P, C.c_int32, C.c_int32, _I32P, _I32P, C.c_int32, _I32P, C.c_int32, C.c_int32,
                                              C.c_float, C.c_float, C.c_uint64, _P, _I32P, _P, _P, _P, _P]),
    "opus_llama_score_continuations_detached": (C.c_int, [_P, _SNAP, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "opus_llama_score_tree_detached": (C.c_int, [_P, _SNAP, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32, _P,
                                                 _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    "opus_generate_lookup": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                       C.c_int32, _I32P, _P, _I32P, C.POINTER(C.c_int64), _P]),
    "opus_llama_verify_step": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _I32P, _P]),
    "opus_debug_last_qkv": (C.c_int, [_P, _P, C.c_int32, _P]),
    "opus_debug_lookup_draft": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "opus_debug_lookup_accept": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _I32P, C.c_int32,
                                           C.c_int32, _I32P, C.c_int32, _P, _P, _I32P, _P]),
    "opus_stream_lag": (C.c_int32, []),
    "opus_stream_begin": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _I32P, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                    C.c_uint64, _P, _P]),
    "opus_stream_run": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _I32P, _I32P, _P]),
    "opus_stream_refill": (C.c_int, [_P, _SNAP, C.c_int32, _I32P, _I32P, _P, _I32P, _P]),
    "opus_stream_end": (C.c_int, [_P, _I32P, _P]),
    "opus_debug_stream_state": (C.c_int, [_P, _I32P, _I32P, _I32P, _I32P, C.POINTER(C.c_int64), C.c_int32, _P]),
    "opus_abi_version": (C.c_int, []),
    "opus_operand_dtype": (C.c_int, []),
    "opus_last_error": (C.c_char_p, []),
    "opus_workspace_bytes": (C.c_int64, [C.POINTER(CConfig)]),
    "opus_ctx_create": (C.c_int, [C.POINTER(CConfig), C.c_int, C.POINTER(_P)]),
    "opus_ctx_destroy": (C.c_int, [_P]),
    "opus_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "opus_weights_ready": (C.c_int, [_P]),
    "opus_lora_merge": (C.c_int, [_P, _P, _P, C.c_float, C.c_int64, C.c_int64, C.c_int32, _P]),
    "opus_fill_synth": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_float, C.c_float,
                                  C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_uint64, C.c_float, C.c_float, _P]),
    "opus_tile_weight": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "opus_quantize_fp8": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "opus_debug_gemm_w8": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "opus_quantize_mxfp4": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "opus_debug_gemm_w4": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "opus_esm2_encode": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "opus_esm2_encode_packed": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.c_int32, _P, _P]),
    "opus_esm2_last_hidden": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "opus_projector_forward": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    "opus_protein_projector": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "opus_switch_projector": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "opus_splice_pad": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32,
                                  _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "opus_llama_prefill": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "opus_llama_decode_step": (C.c_int, [_P, _P, _P, _P]),
    "opus_generate_greedy": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                       C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32), _P]),
    "opus_debug_gemm": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "opus_debug_gemm_norm": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P]),
    "opus_debug_gemm_rope": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "opus_debug_attention": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_float, _P]),
    "opus_debug_attn_prefill": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_int64, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_int32), _P]),
    "opus_generate_sample": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                       C.c_float, C.c_float, C.c_uint64, _P, C.POINTER(C.c_int32), _P]),
    "opus_debug_sample": (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_int32, _P, _P]),
    "opus_timing_enable": (C.c_int, [_P, C.c_int32]),
    "opus_timing_reset": (C.c_int, [_P]),
    "opus_timing_get": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "opus_timing_names": (C.c_int, [C.c_char_p, C.c_int32]),
    "opus_last_logits": (C.c_int, [_P, _P, C.c_int32, _P]),
    "opus_check_error": (C.c_int, [_P, _P]),
    "opus_beam_topk": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "opus_kv_reorder": (C.c_int, [_P, _P, C.c_int32, _P]),
    "opus_beam_sample_topk": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_int32,
                                        _P, _P, _P]),
    "opus_set_sampling_top_k": (C.c_int, [_P, C.c_int32]),
    "opus_set_sampling_warpers": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "opus_set_stop_sequence": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "opus_debug_gemm_slabs": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P]),
    "opus_debug_gemm_plan": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "opus_debug_knob": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "opus_stat": (C.c_int64, [_P, C.c_char_p]),
    "opus_debug_attn_decode": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "opus_debug_attn_decode_form": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "opus_llama_forward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int64, _P]),
    "opus_llama_forward_scratch_bytes": (C.c_int64, [C.POINTER(CConfig), C.c_int32, C.c_int32]),
    "opus_llama_prefix": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_int64), _P]),
    "opus_llama_score_continuations": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int64, _P, _P, _P,
                                                 C.c_int64, _P]),
    "opus_llama_score_scratch_bytes": (C.c_int64, [C.POINTER(CConfig), C.c_int32, C.c_int32]),
    "opus_debug_attn_prefix": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "opus_llama_score_tree": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P,
                                        C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    "opus_llama_score_tree_scratch_bytes": (C.c_int64, [C.POINTER(CConfig), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                        C.c_int32]),
    "opus_llama_dec_rows_cap": (C.c_int64, [C.POINTER(CConfig)]),
    "opus_llama_tree_max_depth": (C.c_int32, []),
    "opus_trie_path_sums": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "opus_set_trie_search": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P]),
    "opus_trie_search_begin": (C.c_int, [_P, _P, C.c_int32, _P]),
    "opus_trie_search_level": (C.c_int, [_P, _TSIO, C.c_int32, _P]),
    "opus_debug_trie_beam_expand": (C.c_int, [_P, _P, C.c_int32, _TSIO, C.c_int32, _P]),
    "opus_debug_attn_tree": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "opus_debug_xent": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "opus_esm2_contacts_packed": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.c_int32, _P, _P, _P, C.c_int64, _P]),
    "opus_esm2_contacts_scratch_bytes": (C.c_int64, [C.POINTER(CConfig), C.POINTER(C.c_int32), C.c_int32]),
    "opus_debug_contacts": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                      _P, C.c_int64, _P]),
    "opus_esm2_lm_head": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "opus_debug_esm2_lm_head": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "opus_generate_scored": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                       C.c_float, C.c_float, C.c_uint64, _P, C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "opus_llama_prefill_fanout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "opus_generate_scored_fanout": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                              C.c_int32, C.c_float, C.c_float, C.c_uint64, _P, C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "opus_debug_argmax_lse": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "opus_set_gen_top_logprobs": (C.c_int, [_P, C.c_int32, _P, _P]),
    "opus_debug_top_logprobs": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "opus_generate_scored_guided": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                              C.c_int32, C.c_float, C.c_float, C.c_uint64, _P, C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "opus_debug_guidance": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P]),
    "opus_set_logits_processors": (C.c_int, [_P, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.c_int32]),
    "opus_debug_logits_process": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                            C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                            _P]),
    "opus_set_token_constraint": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    "opus_debug_token_constraint": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    "opus_debug_gemm_rowscale": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_float, C.POINTER(C.c_int32), _P]),
    "opus_debug_gemm_ln": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libopus_pllm.so (once).  Raises if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OpusError(-100, f"{LIB_PATH} not found: build it with `python opus-pllm_amd/build.py` "
                              "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = l.opus_abi_version()
    if v != ABI_VERSION:
        raise OpusError(-101, f"ABI version mismatch: library {v}, binding {ABI_VERSION}")
    if l.opus_operand_dtype() != (1 if BF16 else 0):
        raise OpusError(-102, f"{LIB_PATH} was not built for {'bf16' if BF16 else 'fp16'} operands")
    _lib = l
    return l


def check(code: int) -> None:
    if code != 0:
        raise OpusError(code, lib().opus_last_error().decode("utf-8", "replace"))
