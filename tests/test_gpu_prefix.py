"""Shared-prefix scoring on the GPU: OpusLlamaForCausalLM.cache_prefix + score_continuations.  The attention kernel alone
(opus_debug_attn_prefix) against fp64, the reference's own forward (tests/golden/forward_micro.npz) split into prompt and
continuation, forward(labels) and the fp32 oracle on the concatenated rows for the three decoder families, what the calls leave
in the context, the bf16 build (tests/bf16_prefix_check.py) and the multiple-choice driver's --rank_options mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import forward_checks as fc
import prefix_checks as pc
from gpu_helpers import record
from test_gpu_forward import LP_ABS_GOLD, LP_ABS_ORACLE, ROW_ALONE_ABS, _llama8b_2layer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATTN_ABS = 4e-3            # attention output vs fp64 (the decode-attention kernel's bound, tests/test_gpu_longctx.py)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_attn_prefix_kernel_vs_fp64(dev):
    o = pc.attn_kernel(dev)
    record("prefix.attn_kernel", o)
    assert max(o.values()) <= ATTN_ABS, o


def test_golden_rows_split_into_prefix_and_continuation(dev):
    o = pc.golden_split(dev)
    record("prefix.golden", o)
    assert o["a"] < LP_ABS_GOLD and o["c"] < LP_ABS_GOLD, o


def _check_fwd(o, lp=LP_ABS_ORACLE):
    assert o["R"] > o["max_batch"], o
    assert o["fwd_abs"] < lp, o
    if "oracle_abs" in o:
        assert o["oracle_abs"] < lp, o
    assert o["zero_pad"] and o["bitwise"] and o["sums_ok"] and o["n_tokens_ok"], o


def test_llama3_8b_widths_vs_forward_and_oracle(dev):
    """Llama-3-8B widths, 2 layers: 6 prompts x 3 continuations = 18 rows > max_batch = 8."""
    o = pc.vs_forward(dev, _llama8b_2layer(), P=6, K=3, seed=11)
    record("prefix.llama8b_2layer", o)
    _check_fwd(o)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,cfg", [("qwen2", opa.micro_qwen()), ("opt", opa.micro_opt())])
def test_families_vs_forward_and_oracle(dev, name, cfg):
    o = pc.vs_forward(dev, cfg, P=5, K=4, seed=12)
    record("prefix.family." + name, o)
    _check_fwd(o)


def test_passes_above_activation_capacity(dev):
    """More continuation positions than one pass of the layer loop holds (max_batch x max_prompt): several passes."""
    cfg = opa.micro(max_batch=2, max_prompt=40)
    o = pc.vs_forward(dev, cfg, P=2, K=12, seed=13, oracle_check=False)                # 24 rows x 8 positions > 80
    record("prefix.passes", o)
    _check_fwd(o)


def test_context_state(dev):
    cfg = opa.micro()
    model = fc.make_model(cfg, dev)
    prompts, conts, ids, mask = pc._prefix_batch(cfg, 3, 2, seed=21)
    src = torch.tensor([0, 0, 1, 1, 2, 2])
    conts = [torch.from_numpy(c) for c in conts]
    tok = torch.tensor([5, 6, 7], dtype=torch.int32)
    # prefix -> decode_logits against prefix -> score (twice) -> decode_logits: bitwise
    model.cache_prefix(ids, attention_mask=mask)
    d0 = model.decode_logits(tok).cpu()
    d0b = model.decode_logits(tok).cpu()
    pre = model.cache_prefix(ids, attention_mask=mask)
    a = model.score_continuations(pre, conts, prefix_rows=src)
    b = model.score_continuations(pre, conts, prefix_rows=src)
    assert torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.logprob, b.logprob)
    d1 = model.decode_logits(tok).cpu()
    c = model.score_continuations(pre, conts, prefix_rows=src)                  # (decode steps keep the prefix)
    d1b = model.decode_logits(tok).cpu()
    assert torch.equal(d0, d1) and torch.equal(d0b, d1b)
    assert torch.equal(a.token_logprobs, c.token_logprobs)
    # cache_prefix is a prefill: its next decode step equals prefill_logits' next one
    dummy = torch.zeros((3, cfg.n_prot_tokens, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=dev)
    emb, m, _ = model._splice(ids, mask, dummy, True)
    model.prefill_logits(emb, m)
    assert torch.equal(model.decode_logits(tok).cpu(), d0)

    def stale(fn):
        p = model.cache_prefix(ids, attention_mask=mask)
        fn(p)
        with pytest.raises(_cabi.OpusError) as e:
            model.score_continuations(p, conts, prefix_rows=src)
        assert e.value.code == -6                                               # OPUS_ESTATE

    gen = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=4)
    stale(lambda p: model.generate(ids, **gen))
    stale(lambda p: model(ids[:, -5:], labels=ids[:, -5:]))
    stale(lambda p: model.cache_prefix(ids, attention_mask=mask))
    stale(lambda p: model.prefill_logits(emb, m))
    stale(lambda p: model.generate(ids, num_beams=2, **gen))                   # (beam search permutes the cache: kv_reorder)
    # a handle of another context
    other = model.new_context()
    p = other.cache_prefix(ids, attention_mask=mask)
    model.cache_prefix(ids, attention_mask=mask)
    with pytest.raises(_cabi.OpusError) as e:
        model.score_continuations(p, conts, prefix_rows=src)
    assert e.value.code == -6
    # a right-padded prefix, continuations above max_prompt, a missing row map
    right = torch.zeros_like(mask)
    right[:, :4] = True
    with pytest.raises(ValueError):
        model.cache_prefix(ids, attention_mask=right)
    p = model.cache_prefix(ids, attention_mask=mask)
    with pytest.raises(_cabi.OpusError) as e:
        model.score_continuations(p, [torch.full((cfg.max_prompt + 1,), 5)] * 3)
    assert e.value.code == -2                                                   # OPUS_ESHAPE
    with pytest.raises(ValueError):
        model.score_continuations(p, conts)
    # right-padded tensor form with a mask = the ragged form
    n = max(len(x) for x in conts)
    t = torch.zeros((len(conts), n), dtype=torch.long)
    tm = torch.zeros((len(conts), n), dtype=torch.bool)
    for i, x in enumerate(conts):
        t[i, : len(x)], tm[i, : len(x)] = x, True
    a2 = model.score_continuations(p, t, prefix_rows=src, attention_mask=tm)
    assert torch.equal(a2.token_logprobs, a.token_logprobs)


def test_row_alone_matches_its_batch_row(dev):
    cfg = _llama8b_2layer()
    model = fc.make_model(cfg, dev)
    prompts, conts, ids, mask = pc._prefix_batch(cfg, 6, 2, seed=31)
    conts = [torch.from_numpy(c) for c in conts]
    src = torch.arange(6).repeat_interleave(2)
    whole = model.score_continuations(model.cache_prefix(ids, attention_mask=mask), conts, prefix_rows=src)
    worst = 0.0
    for r in (0, 5, 11):
        b = int(src[r])
        one = model.score_continuations(model.cache_prefix(ids[b:b + 1, mask[b].nonzero()[0, 0]:]), [conts[r]])
        n = len(conts[r])
        worst = max(worst, float((one.token_logprobs[0, :n] - whole.token_logprobs[r, :n]).abs().max()))
    record("prefix.row_alone", {"alone_abs": worst})
    assert worst < ROW_ALONE_ABS, worst
    del model
    torch.cuda.empty_cache()


def test_bf16_build_prefix():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_prefix_check.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_PREFIX ")][-1]
    o = json.loads(line[len("BF16_PREFIX "):])
    record("prefix.bf16", o)
    assert o["operand_dtype"] == 1, o
    assert max(o["attn"].values()) <= 8 * ATTN_ABS, o
    _check_fwd(o["llama8b"], lp=8 * LP_ABS_ORACLE)


def test_eval_multichoice_rank_options(dev, tmp_path):
    """--rank_options on synthetic:c1_tiny with the question file of tests/test_loader.py: `generated` is one of the four answer
    texts, the one forward(labels) on prompt + answer ranks first."""
    import argparse
    import importlib.util
    from opus_pllm_amd import builder, synth
    spec = importlib.util.spec_from_file_location("eval_multichoice", os.path.join(ROOT, "opus-pllm_amd", "eval_multichoice.py"))
    em = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(em)
    qs = [dict(question="Where is it located?", options=["A) nucleus", "B) membrane", "C) cytosol", "D) secreted"],
               input=synth.synth_protein(40 + 9 * i, i) if i != 2 else "", answer="B) membrane") for i in range(5)]
    inp, out = tmp_path / "q.json", tmp_path / "o.json"
    json.dump(qs, open(inp, "w"))
    args = argparse.Namespace(model_base_path="synthetic:c1_tiny", opus_pllm_weights_path="synthetic", input_path=str(inp),
                              save_path=str(out), temperature=0.0, top_p=0.7, num_beams=1, max_new_tokens=6,
                              switch_projector_type="mlp2x_gelu", load_4bit=False, load_8bit=False, batch_size=4,
                              max_residues=128, max_prompt=256, rank_options=True)
    em.eval_model(args)
    res = json.load(open(out))
    texts = [em.option_text(L) for L in "ABCD"]
    assert len(res) == 5 and all(r["generated"] in texts and len(r["option_logprobs"]) == 4 for r in res), res
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=130, max_prompt=256, max_new_tokens=8)
    if getattr(tok, "chat_template", None) is None:
        from opus_pllm_amd import conversation as conversation_lib
        tok.chat_template = conversation_lib.default_chat_template
    for q, r in zip(qs, res):
        ids = opa.tokenizer_seq_token(em.render_question(q, tok), tok, opa.DEFAULT_SEQ_TOKEN_INDEX, return_tensors="pt")
        lps = []
        for L in "ABCD":
            c = torch.tensor(em.option_ids(tok, L), dtype=torch.long)
            row = torch.cat([ids, c])[None]
            lab = torch.full_like(row, -100)
            lab[0, ids.numel():] = c
            kw = dict(seq=[q["input"]]) if q["input"] else {}
            lps.append(float(model(row, labels=lab, return_logits=False, **kw).token_logprobs.sum()))
        assert np.allclose(lps, r["option_logprobs"], atol=4 * LP_ABS_ORACLE), (lps, r)
        best = int(np.argmax(lps))
        # the choice is forward's argmax (up to a tie within the bound of the two paths)
        assert r["generated"] == texts[best] or lps[texts.index(r["generated"])] > lps[best] - 8 * LP_ABS_ORACLE, (lps, r)
