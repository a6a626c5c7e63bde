"""Host tests (no GPU) of generate(return_dict_in_generate=True, output_*=True): the output classes against transformers'
ModelOutput, compute_transition_scores against transformers' implementation, the counted positions, the C ABI entries and the
cases that raise."""
import ctypes
import os
import re
import types

import pytest
import torch

import opus_pllm_amd as opa  # noqa: F401
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import (GenerateBeamDecoderOnlyOutput, GenerateDecoderOnlyOutput, OpusLlamaForCausalLM,
                                 counted_tokens)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_classes():
    from transformers.generation.utils import GenerateBeamDecoderOnlyOutput as HB, GenerateDecoderOnlyOutput as HD
    return HD, HB


def _same_behaviour(ours, theirs):
    assert list(ours.keys()) == list(theirs.keys())
    assert len(ours) == len(theirs) and list(iter(ours)) == list(iter(theirs))
    a, b = ours.to_tuple(), theirs.to_tuple()
    assert len(a) == len(b) and all(x is y for x, y in zip(a, b))
    for i in range(len(a)):
        assert ours[i] is theirs[i]
    for k in theirs.keys():
        assert ours[k] is theirs[k] and getattr(ours, k) is getattr(theirs, k) and (k in ours)
    with pytest.raises(KeyError):
        ours["attentions"]
    with pytest.raises(KeyError):
        theirs["attentions"]


def test_output_classes_behave_like_model_output():
    HD, HB = _hf_classes()
    seq = torch.arange(6).view(2, 3)
    sc = tuple(torch.randn(2, 5) for _ in range(3))
    for kw in (dict(sequences=seq), dict(sequences=seq, scores=sc), dict(sequences=seq, logits=sc),
               dict(sequences=seq, scores=sc, logits=sc)):
        _same_behaviour(GenerateDecoderOnlyOutput(**kw), HD(**kw))
    ss = torch.randn(2)
    _same_behaviour(GenerateBeamDecoderOnlyOutput(sequences=seq, sequences_scores=ss), HB(sequences=seq, sequences_scores=ss))
    # the extension fields are attributes only: they never enter keys() / to_tuple()
    o = GenerateDecoderOnlyOutput(sequences=seq, token_logprobs=torch.zeros(2, 3), logprob=torch.zeros(2), n_tokens=torch.ones(2))
    assert o.keys() == ["sequences"] and len(o.to_tuple()) == 1 and o.logprob is not None
    with pytest.raises(KeyError):
        o["token_logprobs"]


def _hf_transition(sequences, scores, V, beam_indices=None, normalize_logits=False):
    from transformers.generation.utils import GenerationMixin
    fake = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=V, get_text_config=lambda: types.SimpleNamespace(vocab_size=V)))
    return GenerationMixin.compute_transition_scores(fake, sequences, scores, beam_indices=beam_indices,
                                                     normalize_logits=normalize_logits)


@pytest.mark.parametrize("normalize", [False, True])
def test_compute_transition_scores_matches_transformers(normalize):
    g = torch.Generator().manual_seed(5)
    B, V, n = 4, 37, 6
    scores = []
    for _ in range(n):
        s = torch.randn(B, V, generator=g) * 3
        s[torch.rand(B, V, generator=g) < 0.4] = float("-inf")           # filtered tokens, as sampled scores hold them
        s[:, 0] = torch.randn(B, generator=g)                               # (every row keeps one finite entry)
        scores.append(s)
    scores = tuple(scores)
    seq = torch.randint(0, V, (B, n), generator=g)
    seq[:, 2] = 0
    model = object.__new__(OpusLlamaForCausalLM)
    ours = model.compute_transition_scores(seq, scores, normalize_logits=normalize)
    ref = _hf_transition(seq, scores, V, normalize_logits=normalize)
    assert ours.shape == (B, n) and torch.equal(ours, ref)
    # explicit beam indices, -1 where a beam had stopped (HF's layout)
    bi = torch.randint(0, B, (B, n), generator=g)
    bi[1, 4:] = -1
    bi[3, 5:] = -1
    ours = model.compute_transition_scores(seq, scores, beam_indices=bi, normalize_logits=normalize)
    assert torch.equal(ours, _hf_transition(seq, scores, V, beam_indices=bi, normalize_logits=normalize))


def test_counted_tokens():
    ids = torch.tensor([[5, 7, 9, 2, 2, 2],      # EOS 9 at position 2
                        [1, 1, 1, 1, 1, 1],      # never finishes
                        [4, 8, 3, 6, 2, 2],      # stop sequence (8, 3) ends at position 2
                        [9, 2, 2, 2, 2, 2]])     # EOS first
    assert counted_tokens(ids, [9], [8, 3]).tolist() == [3, 6, 3, 1]
    assert counted_tokens(ids, [], []).tolist() == [6, 6, 6, 6]
    assert counted_tokens(ids[:, :0], [9]).tolist() == [0, 0, 0, 0]


def test_new_symbols_are_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name in ("opus_generate_scored", "opus_debug_argmax_lse"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype == ctypes.c_int and fn.argtypes == _cabi.SIGNATURES[name][1]
    assert lib.opus_abi_version() == 10
    assert len(_cabi.SIGNATURES["opus_generate_scored"][1]) == 18 and len(_cabi.SIGNATURES["opus_debug_argmax_lse"][1]) == 7
    bf = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    assert bf.opus_generate_scored is not None and bf.opus_debug_argmax_lse is not None


def test_workspace_does_not_grow():
    """The outputs are caller memory and the fused pass's scratch is a separate allocation made on first use: a context's
    workspace is the parent's, byte for byte (Llama-3-8B headline configuration and micro)."""
    for cfg, parent in ((opa.llama3_8b(), 6203884288), (opa.micro(), 68627200)):
        cc = _cabi.CConfig.from_config(cfg)
        assert _cabi.lib().opus_workspace_bytes(ctypes.byref(cc)) == parent


def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    return m


@pytest.mark.parametrize("kw", [dict(output_attentions=True), dict(output_hidden_states=True),
                                dict(num_beams=3, output_scores=True), dict(num_beams=2, output_logits=True),
                                dict(num_beams=2, output_token_logprobs=True)])
def test_unsupported_outputs_raise(kw):
    m = _hostless_model()
    ids = torch.ones((1, 4), dtype=torch.long)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, return_dict_in_generate=True, max_new_tokens=2, **kw)
    if "num_beams" in kw:
        assert "sequences_scores" in str(e.value) and "greedy and sampling" in str(e.value)
