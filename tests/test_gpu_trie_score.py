"""Trie scoring on the GPU: OpusLlamaForCausalLM.score_trie.  The attention kernel alone (opus_debug_attn_tree) against fp64, the
reference's own forward (tests/golden/forward_micro.npz) with every labelled span as a one-member trie, the fp32 oracle and
score_continuations on the flat member list for the three decoder families, several passes, what the call leaves in the context,
the bf16 build (tests/bf16_trie_score_check.py) and the annotation driver's --rank_terms mode.  All comparisons are per node /
per token, never per member sum, so no bound scales with the depth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TRIE_MAX_DEPTH, TokenTrie, plan_trie_score
import forward_checks as fc
import prefix_checks as pc
import trie_score_checks as tc
from gpu_helpers import record
from test_gpu_forward import LP_ABS_GOLD, LP_ABS_ORACLE, ROW_ALONE_ABS, _llama8b_2layer
from test_gpu_prefix import ATTN_ABS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_attn_tree_kernel_vs_fp64(dev):
    o = tc.attn_kernel(dev)
    record("trie.attn_kernel", o)
    assert max(o.values()) <= ATTN_ABS, o


def test_golden_spans_as_one_member_tries(dev):
    o = tc.golden_spans(dev)
    record("trie.golden", o)
    assert o["a"] < LP_ABS_GOLD and o["c"] < LP_ABS_GOLD, o


def _check(o, lp=LP_ABS_ORACLE, alone=ROW_ALONE_ABS):
    print(json.dumps(o))
    if "oracle_abs" in o:
        assert o["oracle_abs"] < lp and o["stop_abs"] < lp, o
    assert o["flat_abs"] < alone and o["stop_modes_abs"] < alone, o
    assert o["bitwise"] and o["member_def"] and o["logprob_def"] and o["root_zero"] and o["pad_ok"] and o["topk_ok"] and o["rows_ok"], o


def test_llama3_8b_widths_vs_oracle_and_flat_call(dev):
    """Llama-3-8B widths, 2 layers: one trie shared by 3 prompts, then a trie per prompt."""
    cfg = _llama8b_2layer()
    model = fc.make_model(cfg, dev)
    o = tc.vs_oracle(dev, cfg, P=3, sizes=[9], seed=51, model=model)
    record("trie.llama8b_2layer.shared", o)
    _check(o)
    assert o["rows_full"] == 3 * o["N"] and o["rows_full"] == o["one_pass_rows"][0] and o["rows_bare"] == o["one_pass_rows"][1], o
    o = tc.vs_oracle(dev, cfg, P=3, sizes=[6, 1, 8], seed=52, per_row=True, model=model)
    record("trie.llama8b_2layer.per_row", o)
    _check(o)
    del model
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,cfg", [("qwen2", opa.micro_qwen()), ("opt", opa.micro_opt())])
def test_families_vs_oracle_and_flat_call(dev, name, cfg):
    o = tc.vs_oracle(dev, cfg, P=4, sizes=[25, 3, 14, 1], seed=53, per_row=True)
    record("trie.family." + name, o)
    _check(o)
    assert o["rows_full"] == o["one_pass_rows"][0] and o["rows_bare"] == o["one_pass_rows"][1], o


def test_several_passes(dev):
    """A context whose activation buffers hold 80 rows and tries of more than 80 evaluated nodes per prompt: several passes, the
    ancestors of a pass's first node re-computed."""
    cfg = opa.micro(max_batch=2, max_prompt=40)
    model = fc.make_model(cfg, dev)
    rng = np.random.default_rng(61)
    trie = tc.random_trie(rng, 70, lo=3, hi=6, alphabet=6)
    for stop in (False, True):
        plan = plan_trie_score([trie, trie], stop, 80)
        assert plan.evaluated_nodes > 160 and len(plan.passes) >= 3 and plan.rows_evaluated > plan.evaluated_nodes
    prompts, _, ids, mask = pc._prefix_batch(cfg, 2, 1, 62, lp=(14, 28))
    prefix = model.cache_prefix(ids, attention_mask=mask)
    res = {stop: model.score_trie(prefix, trie, include_stop=stop) for stop in (False, True)}
    node, stop_ref = tc._oracle(cfg, dev, prompts, [trie, trie])
    o = {}
    for stop in (False, True):
        plan = plan_trie_score([trie, trie], stop, 80)
        assert res[stop].rows_evaluated == plan.rows_evaluated
        o["oracle_abs_stop%d" % stop] = float((res[stop].node_logprobs.double().cpu() - node)[:, 1:].abs().max())
    o["stop_abs"] = float((res[True].stop_logprob.double().cpu() - stop_ref).abs().max())
    o["rows"] = [res[False].rows_evaluated, res[True].rows_evaluated]
    record("trie.passes", o)
    print(json.dumps(o))
    assert o["oracle_abs_stop0"] < LP_ABS_ORACLE and o["oracle_abs_stop1"] < LP_ABS_ORACLE and o["stop_abs"] < LP_ABS_ORACLE, o
    big = fc.make_model(opa.micro(max_prompt=64), dev)                                 # one pass: the same numbers within a GEMM's routing
    one = big.score_trie(big.cache_prefix(ids, attention_mask=mask), trie, include_stop=True)
    assert one.rows_evaluated == 2 * trie.n_nodes
    assert float((one.node_logprobs - res[True].node_logprobs).abs().max()) < ROW_ALONE_ABS


def test_context_state(dev):
    cfg = opa.micro()
    model = fc.make_model(cfg, dev)
    prompts, _, ids, mask = pc._prefix_batch(cfg, 3, 1, seed=71)
    trie = tc.random_trie(np.random.default_rng(72), 15)
    tok = torch.tensor([5, 6, 7], dtype=torch.int32)
    # prefix -> decode_logits against prefix -> score_trie (twice) -> decode_logits: bitwise
    model.cache_prefix(ids, attention_mask=mask)
    d0 = model.decode_logits(tok).cpu()
    d0b = model.decode_logits(tok).cpu()
    pre = model.cache_prefix(ids, attention_mask=mask)
    a = model.score_trie(pre, trie, include_stop=True)
    b = model.score_trie(pre, trie, include_stop=True)
    assert torch.equal(a.node_logprobs, b.node_logprobs) and torch.equal(a.logprob, b.logprob)
    d1 = model.decode_logits(tok).cpu()
    c = model.score_trie(pre, trie, include_stop=True)                           # (decode steps keep the prefix)
    d1b = model.decode_logits(tok).cpu()
    assert torch.equal(d0, d1) and torch.equal(d0b, d1b)
    assert torch.equal(a.node_logprobs, c.node_logprobs) and torch.equal(a.stop_logprob, c.stop_logprob)

    def stale(fn):
        p = model.cache_prefix(ids, attention_mask=mask)
        fn(p)
        with pytest.raises(_cabi.OpusError) as e:
            model.score_trie(p, trie)
        assert e.value.code == -6                                                # OPUS_ESTATE

    gen = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=4)
    stale(lambda p: model.generate(ids, **gen))
    stale(lambda p: model(ids[:, -5:], labels=ids[:, -5:]))
    stale(lambda p: model.cache_prefix(ids, attention_mask=mask))
    other = model.new_context()                                                  # a handle of another context
    p = other.cache_prefix(ids, attention_mask=mask)
    model.cache_prefix(ids, attention_mask=mask)
    with pytest.raises(_cabi.OpusError) as e:
        model.score_trie(p, trie)
    assert e.value.code == -6
    # too deep, too long, wrong types; the handle can be scored again afterwards
    p = model.cache_prefix(ids, attention_mask=mask)
    with pytest.raises(_cabi.OpusError) as e:
        model.score_trie(p, TokenTrie([[5] * (TRIE_MAX_DEPTH + 1)], 1))
    assert e.value.code == -2                                                    # OPUS_ESHAPE
    room = cfg.max_prompt + cfg.max_new_tokens - int(p.lengths.max())
    assert 0 < room < TRIE_MAX_DEPTH
    with pytest.raises(_cabi.OpusError) as e:
        model.score_trie(p, TokenTrie([[5] * (room + 1)], 1))
    assert e.value.code == -2
    with pytest.raises(TypeError):
        model.score_trie(p, [[3, 4]])
    with pytest.raises(ValueError):
        model.score_trie(p, TokenTrie.per_row([trie, trie]))
    again = model.score_trie(p, trie, include_stop=True)
    assert torch.equal(again.node_logprobs, a.node_logprobs)
    deep = model.score_trie(p, TokenTrie([[5] * room, [5, 6]], 1), include_stop=True)   # the longest path that fits
    assert torch.isfinite(deep.logprob).all() and deep.rows_evaluated == 3 * (room + 1)


def test_bf16_build_trie_score():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_trie_score_check.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_TRIE_SCORE ")][-1]
    o = json.loads(line[len("BF16_TRIE_SCORE "):])
    record("trie.bf16", o)
    assert o["operand_dtype"] == 1, o
    assert max(o["attn"].values()) <= 8 * ATTN_ABS, o
    _check(o["micro"], lp=8 * LP_ABS_ORACLE, alone=8 * ROW_ALONE_ABS)


def test_eval_ddp_rank_terms(dev, tmp_path):
    """--allowed_terms FILE --rank_terms 3 on synthetic:c1_tiny: no generation, three terms per item in descending order, their
    log-probs those of score_continuations on the same texts behind the same prompt, the first one the best of all terms."""
    import argparse
    import importlib.util
    from opus_pllm_amd import builder, synth
    from opus_pllm_amd.prompt import build_prompt
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    terms = ["GO 0005634 nucleus", "GO 0005634 nuclear lumen", "GO 0005886 plasma membrane", "GO 0005886 membrane raft",
             "GO 0016020 membrane", "GO 0005737 cytoplasm", "GO 0005737", "EC 3.4.21.4", "EC 3.4.21.5", "EC 2.7.11.1", "kinase",
             "GO 0005634 nucleus"]
    tfile, inp, out = tmp_path / "terms.txt", tmp_path / "q.json", tmp_path / "o.json"
    tfile.write_text("\n".join(terms) + "\n")
    qs = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(40 + 9 * i, i), output="x") for i in range(5)]
    json.dump(qs, open(inp, "w"))
    K = 3
    args = argparse.Namespace(model_base_path="synthetic:c1_tiny", opus_pllm_weights_path="synthetic", input_path=str(inp),
                              save_path=str(out), temperature=0.0, top_p=0.7, num_beams=1, max_new_tokens=6,
                              switch_projector_type="mlp2x_gelu", load_4bit=False, load_8bit=False, batch_size=4, max_residues=128,
                              max_prompt=None, collective_timeout=60, use_input_embed=False, stop_at_hashes=False, inflight=1,
                              save_logprobs=False, dump_logits=None, allowed_terms=str(tfile), allowed_separator=None,
                              allowed_prefix="", rank_terms=K, rank_with_stop=False)
    ddp.eval_model(args)
    res = json.load(open(out))
    assert len(res) == 5 and all(len(r["ranked_terms"]) == K and r["generated"] == r["ranked_terms"][0][0] for r in res), res
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=130, max_prompt=96, max_new_tokens=8)
    trie = TokenTrie.from_strings(tok, terms, end_token_id=tok.eos_token_id)
    assert len(trie.member_strings) == len(set(terms))
    conts = [torch.tensor(m, dtype=torch.long) for m in trie.member_ids]
    worst = 0.0
    for q, r in zip(qs, res):
        ids = opa.tokenizer_seq_token(build_prompt(q["instruction"], str(inp)), tok, opa.DEFAULT_SEQ_TOKEN_INDEX, return_tensors="pt")
        prefix = model.cache_prefix(ids[None], seq=[q["input"]])
        lps = model.score_continuations(prefix, conts, prefix_rows=torch.zeros(len(conts), dtype=torch.long)).logprob.cpu().tolist()
        got = r["ranked_terms"]
        assert all(t in trie.member_strings for t, _ in got) and len({t for t, _ in got}) == K, got
        assert all(got[k][1] >= got[k + 1][1] for k in range(K - 1)), got
        for t, lp in got:
            worst = max(worst, abs(lp - lps[trie.member_strings.index(t)]))
        assert max(lps) - got[0][1] < 4 * LP_ABS_ORACLE, (lps, got)                    # the first one is the best of all terms
    record("trie.rank_terms", {"logprob_abs": worst})
    print(json.dumps({"rank_terms_logprob_abs": worst}))
    assert worst < 4 * LP_ABS_ORACLE, worst
