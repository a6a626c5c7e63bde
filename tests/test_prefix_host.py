"""Host-side parts of shared-prefix scoring that need no GPU: the C ABI additions of both library builds and the scratch sizing
of opus_llama_score_continuations."""
import ctypes as C
import os

import pytest

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("opus_llama_prefix", "opus_llama_score_continuations", "opus_llama_score_scratch_bytes", "opus_debug_attn_prefix")


@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_new_symbols_exported_and_bound(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    for name in NEW:
        assert name in _cabi.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.opus_abi_version() == 10
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    for name in NEW:
        assert name + "(" in header


def _expected(cfg, R, n):
    """Table words of one pass (prefix-row offsets, row list, position bases, workgroup pairs, gather index) + the gathered fp32
    rows and the fp16 logits slab of a loss-only scoring chunk (tests/test_forward_host.py), each 256-byte aligned."""
    up = lambda b: -(-b // 256) * 256                                                   # noqa: E731
    Md = max(cfg.max_batch * cfg.max_prompt, -(-cfg.max_batch // 16) * 16)
    Rg = min(R, Md // n)
    G = cfg.dec_heads // cfg.dec_kv_heads
    words = cfg.max_batch + 1 + 2 * Rg + 2 * ((Rg * G * n) // 128 + cfg.max_batch) + Rg * n
    cap = (128 * 2 ** 20) // (2 * cfg.dec_vocab)
    cap = cap // 64 * 64 if cap >= 64 else max(cap, 1)
    chunk = min(Rg * n, cap)
    return up(4 * words) + up(chunk * cfg.dec_dim * 4) + up(chunk * cfg.dec_vocab * 2)


def test_score_scratch_bytes():
    lib = _cabi.lib()
    big = opa.llama3_8b(max_batch=64, max_enc_tokens=66, max_prompt=110, max_new_tokens=16)
    cc = _cabi.CConfig.from_config(big)
    # the bench shape: 256 rows x 6 positions, one pass; 1536 scored rows -> chunks of 512 at V = 128 256
    assert lib.opus_llama_score_scratch_bytes(C.byref(cc), 256, 6) == _expected(big, 256, 6)
    words = 65 + 512 + 2 * (256 * 4 * 6 // 128 + 64) + 1536
    assert _expected(big, 256, 6) == -(-words * 4 // 256) * 256 + 512 * 4096 * 4 + 512 * 128256 * 2
    micro = opa.micro()
    mc = _cabi.CConfig.from_config(micro)
    for R, n in ((1, 1), (7, 5), (30, 48), (500, 3)):                                # (500 x 3 > 8 x 48: passes of 128 rows)
        assert lib.opus_llama_score_scratch_bytes(C.byref(mc), R, n) == _expected(micro, R, n), (R, n)
    assert _expected(micro, 1, 1) == 256 + 256 + 256                                 # 28 words; 1 x 64 fp32; 1 x 96 fp16
    for R, n in ((0, 4), (-1, 4), (4, 0), (4, micro.max_prompt + 1)):
        assert lib.opus_llama_score_scratch_bytes(C.byref(mc), R, n) == -1, (R, n)
    bad = _cabi.CConfig.from_config(micro)
    bad.dec_heads = 0
    assert lib.opus_llama_score_scratch_bytes(C.byref(bad), 4, 4) == -1
