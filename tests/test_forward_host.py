"""Host-side parts of forward(labels=...) that need no GPU: the C ABI additions of both library builds, the scratch sizing,
the timing names, the reference fixture's self-consistency, the mask rules and the HF-shaped output object."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import CausalLMOutput, _check_forward_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("opus_llama_forward", "opus_llama_forward_scratch_bytes", "opus_debug_xent")


@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_new_symbols_exported_and_bound(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    for name in NEW:
        assert name in _cabi.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.opus_abi_version() == 10


def test_scratch_sizing_and_workspace():
    lib = _cabi.lib()
    cfg = opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=136, max_new_tokens=16)
    cc = _cabi.CConfig.from_config(cfg)
    H, V = cfg.dec_dim, cfg.dec_vocab
    loss_only = lib.opus_llama_forward_scratch_bytes(C.byref(cc), 2048, 0)
    # chunk = the largest multiple of 64 rows whose fp16 logits fit 128 MiB (512 rows at V = 128 256) + those rows in fp32
    rows = (128 * 2 ** 20 // (2 * V)) // 64 * 64
    assert rows == 512
    assert loss_only == rows * H * 4 + rows * V * 2
    assert lib.opus_llama_forward_scratch_bytes(C.byref(cc), 100, 0) == 100 * H * 4 + -(-100 * V * 2 // 256) * 256
    assert lib.opus_llama_forward_scratch_bytes(C.byref(cc), 64 * 136, 1) == 64 * 136 * H * 4     # logits in the caller's buffer
    assert lib.opus_llama_forward_scratch_bytes(C.byref(cc), 0, 0) == 0
    assert lib.opus_llama_forward_scratch_bytes(C.byref(cc), -1, 0) == -1
    micro = _cabi.CConfig.from_config(opa.micro())
    assert lib.opus_llama_forward_scratch_bytes(C.byref(micro), 5, 0) == 1280 + 1024     # 5 x 64 fp32, 5 x 96 fp16 (256-aligned)


def test_timing_names_add_xent_and_score_at_the_end():
    buf = C.create_string_buffer(512)
    assert _cabi.lib().opus_timing_names(buf, 512) == 0
    classes, phases = buf.value.decode().split(";")
    assert classes.split(",")[-1] == "xent"
    assert phases.split(",") == ["encode", "project", "splice", "prefill", "decode", "other", "score"]


def test_forward_fixture_is_self_consistent():
    g = np.load(os.path.join(ROOT, "tests", "golden", "forward_micro.npz"))
    for tag in "abc":
        lp = g[tag + ".token_logprobs"]
        lab = g[tag + ".labels_out"]
        cnt = np.zeros_like(lab, dtype=bool)
        cnt[:, 1:] = lab[:, 1:] != -100
        assert int(cnt.sum()) == int(g[tag + ".n_tokens"]) > 0
        assert (lp[~cnt] == 0).all() and (lp[cnt] < 0).all()
        assert abs(float(g[tag + ".loss"]) + lp[cnt].mean()) < 1e-5 * abs(float(g[tag + ".loss"]))
        assert g[tag + ".logits"].shape[:2] == lab.shape
    assert g["b.logits"].shape[1] == int(g["b.max_length"]) < g["a.logits"].shape[1]       # the truncation bites
    assert "d.loss" not in g.files


def test_mask_rules():
    ok = np.array([[1, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=bool)
    _check_forward_mask(ok, None)                                           # right-padded / unpadded / empty rows
    with pytest.raises(ValueError, match="hole"):
        _check_forward_mask(np.array([[1, 0, 1, 0]], dtype=bool), None)
    left = np.array([[0, 1, 1, 1], [1, 1, 1, 1]], dtype=bool)
    with pytest.raises(ValueError, match="position_ids"):
        _check_forward_mask(left, None)
    pos = np.cumsum(left, axis=1) - 1
    _check_forward_mask(left, pos)
    with pytest.raises(ValueError, match="position_ids"):
        _check_forward_mask(left, np.tile(np.arange(4), (2, 1)))            # HF's arange positions: not what the kernels do


def test_output_object_is_indexed_like_hf():
    loss, logits = torch.tensor(1.5), torch.zeros(1, 2, 3)
    o = CausalLMOutput(loss=loss, logits=logits, token_logprobs=torch.zeros(1, 2), n_tokens=1)
    assert o[0] is loss and o[1] is logits and o["logits"] is logits and o.to_tuple() == (loss, logits)
    assert list(o.keys()) == ["loss", "logits"] and o.past_key_values is None
    n = CausalLMOutput(loss=None, logits=logits)
    assert n.to_tuple() == (logits,) and n[0] is logits
    with pytest.raises(KeyError):
        n["loss"]
