"""Host tests (no GPU) of generate(guidance_scale=...): the paired-row restatement (tests/guidance_ref.py) against the installed
transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, the protein-free twin and the common-length padding, every error
that is raised before the device is touched, and the C ABI entries."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import (OpusLlamaForCausalLM, pad_left_common, protein_free_twin, spliced_length)
import guidance_ref as gr
import logits_proc_ref as lpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = opa.DEFAULT_SEQ_TOKEN_INDEX

SCORES_ABS = 1e-4          # restatement vs transformers (measured <= 1.2e-5 on this kind of model; ~8x for other BLAS builds)
MIN_GAP = 1e-3             # every step of every case is decided by more than this: no case can pass on a tie


def _tiny_llama(seed):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    V, H = 40, 32
    hf = LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=H, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                      num_key_value_heads=2, max_position_embeddings=64)).eval()
    with torch.no_grad():
        for prm in hf.parameters():
            prm.mul_(4.0)                                             # sharper distributions, as tests/test_host.py
    return hf, V, H


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("g", [1.5, 3.0])
def test_restatement_matches_transformers(g, seed):
    """generate(inputs_embeds, guidance_scale, negative_prompt_ids, negative_prompt_attention_mask) of the installed transformers
    against the paired-row form: ids equal, scores within SCORES_ABS, for plain greedy, an EOS id, repetition_penalty,
    no_repeat_ngram_size and min_new_tokens; one conditional and one negative row are left-padded."""
    pytest.importorskip("transformers")
    hf, V, H = _tiny_llama(100 + seed)
    B, T, Tn, N = 3, 6, 5, 9
    emb = torch.randn(B, T, H)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :2] = 0                                                   # a left-padded conditional row
    neg = torch.randint(1, V, (B, Tn))
    nmask = torch.ones(B, Tn, dtype=torch.long)
    nmask[2, :3] = 0                                                  # a left-padded negative row
    tok_emb = hf.get_input_embeddings()

    def logits_fn(e, m):
        pos = (m.long().cumsum(-1) - 1).clamp(min=0)
        with torch.no_grad():
            return hf(inputs_embeds=e, attention_mask=m.long(), position_ids=pos).logits[:, -1].float()

    def embed_fn(ids):
        with torch.no_grad():
            return tok_emb(ids)

    def run_hf(**kw):
        with torch.no_grad():
            return hf.generate(inputs_embeds=emb, attention_mask=mask, guidance_scale=g, negative_prompt_ids=neg,
                               negative_prompt_attention_mask=nmask, do_sample=False, max_new_tokens=N, use_cache=True,
                               pad_token_id=0, output_scores=True, return_dict_in_generate=True, **kw)

    free = run_hf(eos_token_id=None)
    eos = [int(free.sequences[0, 3])]
    cases = {"plain": (dict(eos_token_id=None), dict()),
             "eos": (dict(eos_token_id=eos), dict(eos=eos)),
             "penalty": (dict(eos_token_id=None, repetition_penalty=1.3), dict(penalty=1.3)),
             "ngram": (dict(eos_token_id=None, no_repeat_ngram_size=2), dict(ngram=2)),
             "min_new": (dict(eos_token_id=eos, min_new_tokens=6), dict(eos=eos, min_new=6))}
    with torch.no_grad():
        ec, eu = emb, tok_emb(neg)
    for tag, (hkw, rkw) in cases.items():
        want = free if tag == "plain" else run_hf(**hkw)
        e = rkw.get("eos", [])
        proc = None
        if any(k in rkw for k in ("penalty", "ngram", "min_new")):
            proc = lambda s, hist, rkw=rkw: lpr.process(s, hist, eos=rkw.get("eos", []), penalty=rkw.get("penalty"),   # noqa: E731
                                                        ngram=rkw.get("ngram", 0), min_new=rkw.get("min_new", 0))
        got = gr.guided_generate(logits_fn, embed_fn, ec, mask, eu, nmask, g, N, eos=e, pad_id=0, process=proc)
        assert got["ids"].shape == tuple(want.sequences.shape), (tag, got["ids"], want.sequences)
        assert torch.equal(got["ids"], want.sequences), (tag, got["ids"], want.sequences)
        assert len(want.scores) == got["scores"].shape[0]
        worst = 0.0
        for t, ws in enumerate(want.scores):
            ours = got["scores"][t]
            assert torch.equal(torch.isinf(ours), torch.isinf(ws.float())), (tag, t)
            fin = torch.isfinite(ours)
            # (transformers computes a finished row's scores too; the restatement does the same until every row has finished)
            worst = max(worst, float((ours[fin].double() - ws.float()[fin].double()).abs().max()))
        gap = float(got["gaps"].min())
        print(f"guidance_host g={g} seed={seed} {tag}: scores_abs={worst:.3e} min_gap={gap:.3e}")
        assert gap > MIN_GAP, (tag, gap)
        assert worst <= SCORES_ABS, (tag, worst)
        if tag == "eos":
            assert int((got["ids"][0] == eos[0]).sum()) == 1 and bool((got["ids"][0, 4:] == 0).all()), got["ids"]   # row 0 ends early
        if tag == "min_new":
            assert not bool((got["ids"][:, :6] == eos[0]).any()), got["ids"]


def test_combine_twin_is_hf_expression():
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor  # noqa: F401
    g = torch.Generator().manual_seed(5)
    c, u = torch.randn(4, 33, generator=g) * 4, torch.randn(4, 33, generator=g) * 4
    for s in (0.0, 0.5, 1.5, 3.0, 7.5):
        lc, lu = torch.log_softmax(c, -1), torch.log_softmax(u, -1)
        want = s * (lc - lu) + lu                                     # (logits_process.py: guidance_scale * (scores - uncond) + uncond)
        assert torch.equal(gr.combine(c, u, s), want)
        ref = gr.combine(c, u, s, torch.float64)
        viaL = gr.combine_with_lse(c.double(), u.double(), torch.logsumexp(c.double(), 1), torch.logsumexp(u.double(), 1), s)
        assert float((viaL - ref).abs().max()) < 1e-12
    same = gr.combine(c, c.clone(), 3.0)
    assert torch.equal(same, torch.log_softmax(c, -1))               # g * 0 + u == u


def test_protein_free_twin_and_padding():
    ids = torch.tensor([[0, 0, 1, 7, 8, 9],                           # no placeholder, left-padded by 2
                        [1, 5, SEQ, 6, 7, 8],                         # one
                        [1, SEQ, 4, SEQ, 5, 6]])                      # two
    mask = torch.tensor([[0, 0, 1, 1, 1, 1], [1] * 6, [1] * 6]).bool()
    nid, nm = protein_free_twin(ids, mask)
    assert nid.dtype == torch.int64 and nm.dtype == torch.bool and nid.shape == (3, 5)
    assert nid.tolist() == [[0, 1, 7, 8, 9], [1, 5, 6, 7, 8], [0, 1, 4, 5, 6]]
    assert nm.tolist() == [[False, True, True, True, True], [True] * 5, [False, True, True, True, True]]
    assert not bool((nid == SEQ).any())
    # no mask: every position counts; a masked-out placeholder is dropped with its position
    nid2, nm2 = protein_free_twin(torch.tensor([[SEQ, 3, 4]]), None)
    assert nid2.tolist() == [[3, 4]] and nm2.tolist() == [[True, True]]
    with pytest.raises(ValueError):
        protein_free_twin(torch.tensor([[SEQ, SEQ]]), None)
    # lengths after the splice: a placeholder stands for n_prot_tokens positions
    assert spliced_length(ids, mask, 4) == 6 + 2 * 3
    assert spliced_length(nid, nm, 4) == 5
    assert spliced_length(ids, mask, 4, max_length=9) == 9
    # common-length padding: both sets moved to the right end, zeros and mask 0 in front, conditional rows first
    a = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 3, 2) + 1
    am = torch.tensor([[0, 1, 1], [1, 1, 1]], dtype=torch.uint8)
    b = -(torch.arange(2 * 5 * 2, dtype=torch.float32).view(2, 5, 2) + 1)
    bm = torch.tensor([[1] * 5, [0, 0, 1, 1, 1]], dtype=torch.uint8)
    for (x, xm, y, ym) in ((a, am, b, bm), (b, bm, a, am)):
        out, m = pad_left_common(x, xm, y, ym)
        T = 5
        assert out.shape == (4, T, 2) and m.shape == (4, T) and m.dtype == torch.uint8
        assert torch.equal(out[:2, T - x.shape[1]:], x) and torch.equal(out[2:, T - y.shape[1]:], y)
        assert float(out[:2, :T - x.shape[1]].abs().sum()) == 0 and float(out[2:, :T - y.shape[1]].abs().sum()) == 0
        assert torch.equal(m[:2, T - x.shape[1]:], xm) and torch.equal(m[2:, T - y.shape[1]:], ym)
        assert int(m[:2, :T - x.shape[1]].sum()) == 0 and int(m[2:, :T - y.shape[1]].sum()) == 0
    e, em = gr.pad_left(a, am, b, bm)                                 # the restatement pads the same way
    o, om = pad_left_common(a, am, b, bm)
    assert torch.equal(e, o) and torch.equal(em, om.bool())


def _hostless_model(**cfg_kw):
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro(**cfg_kw)
    return m


@pytest.mark.parametrize("g", [float("nan"), float("inf"), -float("inf"), "2", True, [2.0]])
def test_scale_must_be_a_finite_number(g):
    m = _hostless_model()
    with pytest.raises(ValueError) as e:
        m.generate(torch.ones((1, 4), dtype=torch.long), max_new_tokens=2, guidance_scale=g)
    assert "guidance_scale" in str(e.value)


def test_negative_prompt_errors():
    m = _hostless_model()
    ids = torch.ones((2, 4), dtype=torch.long)
    with pytest.raises(ValueError) as e:                              # another row count
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, negative_prompt_ids=torch.ones((3, 4), dtype=torch.long))
    assert "negative_prompt_ids" in str(e.value)
    with pytest.raises(ValueError) as e:                              # a placeholder
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, negative_prompt_ids=torch.tensor([[1, SEQ, 3], [1, 2, 3]]))
    assert "<seq>" in str(e.value)
    with pytest.raises(ValueError) as e:                              # a mask of another shape
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, negative_prompt_ids=torch.ones((2, 3), dtype=torch.long),
                   negative_prompt_attention_mask=torch.ones((2, 4), dtype=torch.long))
    assert "negative_prompt_attention_mask" in str(e.value)


def test_capacity_errors():
    m = _hostless_model(max_batch=3)
    with pytest.raises(_cabi.OpusError) as e:
        m.generate(torch.ones((2, 4), dtype=torch.long), max_new_tokens=2, guidance_scale=2.0)
    assert e.value.code == -2 and "max_batch=3" in str(e.value) and "2 x 2" in str(e.value)
    m = _hostless_model(max_batch=4)
    too_long = torch.ones((2, m.cfg.max_prompt + 1), dtype=torch.long)
    with pytest.raises(_cabi.OpusError) as e:                         # the negative prompt alone is too long
        m.generate(torch.ones((2, 4), dtype=torch.long), max_new_tokens=2, guidance_scale=2.0, negative_prompt_ids=too_long)
    assert e.value.code == -2 and f"max_prompt={m.cfg.max_prompt}" in str(e.value)
    ids = torch.ones((1, m.cfg.max_prompt - 1), dtype=torch.long)     # the spliced conditional row is
    ids[0, 2] = SEQ
    if m.cfg.n_prot_tokens > 2:
        with pytest.raises(_cabi.OpusError) as e:
            m.generate(ids, ["ACD"], max_new_tokens=2, guidance_scale=2.0)
        assert e.value.code == -2 and "max_prompt" in str(e.value)


def test_combinations_not_built_raise():
    m = _hostless_model()
    ids = torch.ones((1, 4), dtype=torch.long)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, num_beams=2)
    assert "num_beams" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, do_sample=True, seed=1, num_return_sequences=2)
    assert "num_return_sequences" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, max_new_tokens=2, guidance_scale=2.0, prefix=object())
    assert "prefix" in str(e.value)


def test_new_symbols_are_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name, nargs in (("opus_generate_scored_guided", 19), ("opus_debug_guidance", 6)):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        fn = getattr(lib, name)
        assert fn.restype == ctypes.c_int and fn.argtypes == _cabi.SIGNATURES[name][1]
    assert lib.opus_abi_version() == 10
    bf = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    assert bf.opus_generate_scored_guided is not None and bf.opus_debug_guidance is not None
    # both refuse a null context before anything touches a device
    assert lib.opus_debug_guidance(None, None, 1, 1, 1.5, None) != 0
    assert lib.opus_generate_scored_guided(None, None, None, 1, 1, 1.5, 1, None, 0, 0, 0.0, 1.0, 0, None, None, None, None, None, None) != 0


def test_timing_class_guidance_is_listed():
    buf = ctypes.create_string_buffer(512)
    _cabi.check(_cabi.lib().opus_timing_names(buf, 512))
    classes = buf.value.decode().split(";")[0].split(",")
    assert classes[-1] == "xent" and classes[-3:] == ["mlm", "logitproc", "xent"], classes
    assert classes.index("guidance") == classes.index("constraint") + 1 == classes.index("mlm") - 1, classes


def test_kernel_source_is_built_into_both_libraries():
    import importlib.util
    spec = importlib.util.spec_from_file_location("opus_build", os.path.join(ROOT, "opus-pllm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "guidance.hip" in b.SOURCES and any("guidance_".startswith(k) or k == "guidance_" for k in b.NO_SCRATCH)
