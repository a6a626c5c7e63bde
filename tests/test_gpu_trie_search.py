"""Trie search on the GPU: OpusLlamaForCausalLM.search_trie.  The expand kernel alone (opus_debug_trie_beam_expand) against the CPU
twin (tests/trie_search_ref.py) - exact ids, parents, states and members, bitwise scores; the whole call against score_trie on the
same prefix and trie for the three decoder families and the Llama-3-8B widths, per NODE under ROW_ALONE_ABS (one computation on
two launch shapes), never per member sum; groups, detached and attached prefixes, a second context, what the call leaves in the
context; the bf16 build (tests/bf16_trie_search_check.py) and the annotation driver's --search_terms mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TokenTrie
import forward_checks as fc
import prefix_checks as pc
import trie_score_checks as tc
import trie_search_checks as ts
from gpu_helpers import record
from test_gpu_forward import ROW_ALONE_ABS, _llama8b_2layer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kernel_models(dev):
    """Contexts of 128 decoder rows for the kernel test: the micro vocabulary and Llama-3's (micro widths: only V matters)."""
    return {V: fc.make_model(opa.micro(dec_vocab=V, max_batch=128), dev) for V in (96, 128256)}


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("K", [1, 2, 8, 16])
@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("V", [96, 128256])
def test_expand_kernel_vs_twin(kernel_models, V, P, K):
    o = ts.expand_kernel(kernel_models[V], V, P, K, seed=1000 * K + 10 * P + (V > 96))
    record(f"trie_search.kernel.V{V}.P{P}.K{K}", o)
    print(json.dumps(o))
    assert o["ok"], o["why"]
    assert o["launches"] == 4 and o["stop_abs"] < 1e-5, o
    if V > 8192:
        assert o["wide_states"] >= 2, o                       # the root of more than 4 096 children, first level and later
    if K > 1:
        assert o["dead"] > 0, o
    if K >= 8 and P == 8:
        assert o["ties"] > 0, o


# ------------------------------------------------------------------------------------------------ end to end
def _check(o, alone=ROW_ALONE_ABS):
    print(json.dumps(o))
    assert o["beams_compared"] > 0 and o["node_abs"] < alone, o
    if o["stop"]:
        assert o["stops_compared"] > 0 and o["stop_abs"] < alone, o
    assert o["bitwise"] and o["no_nan"] and o["pad_ok"] and o["sorted_ok"], o
    assert o["rank_mismatch"] == 0 and o["topk_mismatch"] == 0, o
    assert 4 * o["decisive"] >= 3 * o["ranks"], o            # at least 3 of 4 compared ranks decide


@pytest.mark.parametrize("name,cfg", [("llama", opa.micro(max_batch=16)), ("qwen2", opa.micro_qwen(max_batch=16)),
                                      ("opt", opa.micro_opt(max_batch=16))])
def test_families_vs_score_trie(dev, name, cfg):
    """A beam wide enough (exhaustive: score_trie's top-k) and a beam of 2 on a trie wider than 2, with and without the stop term."""
    model = fc.make_model(cfg, dev)
    rng = np.random.default_rng(81)
    trie = tc.random_trie(rng, 14, hi=4, alphabet=5)
    assert max(sum(1 for v in range(1, trie.n_nodes + 1) if trie.node_depth[v] == d) for d in range(1, 5)) <= 16     # 16 beams hold a level
    assert sum(1 for v in trie.children[0].values() if trie.children[v]) > 2                                            # 2 beams do not
    for stop in (False, True):
        o, res, sc = ts.vs_score_trie(model, cfg, 1, [trie], K=16, top=4, stop=stop, seed=82, alone=ROW_ALONE_ABS)
        record(f"trie_search.{name}.wide.stop{int(stop)}", o)
        _check(o)
        assert o["exhaustive"] == [True], o
        o, res, sc = ts.vs_score_trie(model, cfg, 3, [trie] * 3, K=2, top=2, stop=stop, seed=83, alone=ROW_ALONE_ABS)
        record(f"trie_search.{name}.beam2.stop{int(stop)}", o)
        _check(o)
        assert o["exhaustive"] == [False] * 3, o
    del model


def test_llama3_8b_widths_per_row_and_top_above_members(dev):
    """Llama-3-8B widths, 2 layers (8 decoder rows, members of at most 4 ids): per-row tries of different sizes, one of them a
    one-member trie, top above its member count; 3 prompts x 4 beams run as two groups."""
    cfg = _llama8b_2layer()
    model = fc.make_model(cfg, dev)
    rng = np.random.default_rng(91)
    tries = [tc.random_trie(rng, 9, hi=4, alphabet=4), TokenTrie([[7, 9]], tc.END), tc.random_trie(rng, 5, hi=3, alphabet=4)]
    for stop in (False, True):
        o, res, sc = ts.vs_score_trie(model, cfg, 3, tries, K=4, top=4, stop=stop, seed=92, alone=ROW_ALONE_ABS, per_row=True)
        record(f"trie_search.llama8b_2layer.per_row.stop{int(stop)}", o)
        _check(o)
        assert res.member_index[1].tolist() == [0, -1, -1, -1] and bool(res.exhaustive[1]), res.member_index
        assert res.logprob[1, 1:].tolist() == [float("-inf")] * 3 and res.n_members.tolist() == [len(t.member_ids) for t in tries]
    del model
    torch.cuda.empty_cache()


def _handle_rows(pre, lo, hi):
    """Rows lo .. hi - 1 of a detached handle as a handle of their own."""
    import ctypes as C
    from opus_pllm_amd.model import OpusPrefix
    sub = OpusPrefix(pre._owner, pre._epoch, pre._last_rows[lo:hi].contiguous(), pre.lengths[lo:hi], slots=pre.slots)
    sub._k, sub._v, sub._kstart = pre._k[:, lo:hi].contiguous(), pre._v[:, lo:hi].contiguous(), pre._kstart[lo:hi].contiguous()
    sub._h_kstart = (C.c_int32 * (hi - lo))(*sub._kstart.cpu().tolist())
    return sub


def test_groups_contexts_and_prefix_forms(dev):
    """max_batch small: the prompts run in several groups; a group of the same row count gives bitwise the single-group rows,
    another row count stays inside the per-node bound.  Detached and attached prefixes and a context of new_context() agree
    bitwise (the same launches)."""
    rng = np.random.default_rng(101)
    trie = tc.random_trie(rng, 16, hi=4, alphabet=5)
    cfg8, cfg4 = opa.micro(max_batch=8), opa.micro(max_batch=4)
    batch = pc._prefix_batch(cfg8, 4, 1, 102)
    big, small = fc.make_model(cfg8, dev), fc.make_model(cfg4, dev)
    kw = dict(num_beams=2, top=2, include_stop=True, return_trace=True)
    pre = big.cache_prefix(batch[2], attention_mask=batch[3], detach=True)
    one = big.search_trie(pre, trie, **kw)                                        # 4 prompts x 2 beams: one group of 8 rows
    pre_s = small.cache_prefix(batch[2], attention_mask=batch[3], detach=True)
    two = small.search_trie(pre_s, trie, **kw)                                    # two groups of 4 rows
    worst = 0.0
    for model, handle, res in ((big, pre, one), (small, pre_s, two)):
        want_all = model.score_trie(handle, trie, include_stop=True).node_logprobs.cpu()
        for lv in res.trace:
            alive = lv["alive"]
            want = want_all[lv["prompt"][alive], lv["node"][alive].long()]
            worst = max(worst, float((lv["edge_logprob"][alive] - want).abs().max()) if alive.any() else 0.0)
    record("trie_search.groups", {"node_abs": worst})
    assert worst < ROW_ALONE_ABS
    # the same row count per group: 8 prompts x 2 beams on the 8-row context are two groups of 8 rows; each is bitwise what its
    # four prompts give as a call of their own (the handle's rows lo .. lo + 3: the same K / V, last rows and first slots)
    b8 = pc._prefix_batch(cfg8, 8, 1, 103)
    pre8 = big.cache_prefix(b8[2], attention_mask=b8[3], detach=True)
    both = big.search_trie(pre8, trie, **kw)
    assert both.rows_decoded > 0 and both.member_index.shape == (8, 2)
    for lo in (0, 4):
        part = big.search_trie(_handle_rows(pre8, lo, lo + 4), trie, **kw)
        assert torch.equal(part.member_index, both.member_index[lo: lo + 4]) and torch.equal(part.logprob, both.logprob[lo: lo + 4])
        assert torch.equal(part.exhaustive, both.exhaustive[lo: lo + 4])
    # attached prefix: detached on the fly; a second context takes the detached handle
    live = big.cache_prefix(batch[2], attention_mask=batch[3])
    assert not live.detached
    att = big.search_trie(live, trie, **kw)
    assert live.detached and torch.equal(att.member_index, one.member_index) and torch.equal(att.logprob, one.logprob)
    other = big.new_context()
    oth = other.search_trie(pre, trie, **kw)
    assert torch.equal(oth.member_index, one.member_index) and torch.equal(oth.logprob, one.logprob)
    again = big.search_trie(pre, trie, **kw)
    assert torch.equal(again.member_index, one.member_index) and torch.equal(again.logprob, one.logprob) and again.levels == one.levels


def test_context_state(dev):
    """What the call leaves behind: generate() afterwards gives the ids of a fresh context; another live handle of the context is
    stale exactly as after generate(prefix=...)."""
    cfg = opa.micro()
    _, _, ids, mask = pc._prefix_batch(cfg, 3, 1, seed=111)
    trie = tc.random_trie(np.random.default_rng(112), 12, hi=4)
    gen = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=5)
    fresh = fc.make_model(cfg, dev).generate(ids, **gen)
    model = fc.make_model(cfg, dev)
    pre = model.cache_prefix(ids, attention_mask=mask, detach=True)
    model.search_trie(pre, trie, num_beams=2, top=2)
    assert torch.equal(model.generate(ids, **gen), fresh)
    model.search_trie(pre, trie, num_beams=2, top=2, include_stop=True)
    assert torch.equal(model.generate(ids, **gen), fresh)

    def stale_code(fn):
        bystander = model.cache_prefix(ids, attention_mask=mask)                   # a live handle that is NOT handed to the call
        fn()
        with pytest.raises(_cabi.OpusError) as e:
            model.score_trie(bystander, trie)
        return e.value.code

    suffix = torch.tensor([[5, 6]] * 3)
    after_generate = stale_code(lambda: model.generate(suffix, prefix=pre, pad_token_id=2, do_sample=False, max_new_tokens=2))
    after_search = stale_code(lambda: model.search_trie(pre, trie, num_beams=2, top=1))
    assert after_generate == after_search == -6
    # the refusals leave the context usable
    with pytest.raises(ValueError):
        model.search_trie(pre, trie, num_beams=2, top=3)
    res = model.search_trie(pre, trie, num_beams=8, top=3)
    assert res.exhaustive.all() and (res.member_index >= 0).all()


def test_bf16_build_trie_search():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_trie_search_check.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_TRIE_SEARCH ")][-1]
    o = json.loads(line[len("BF16_TRIE_SEARCH "):])
    record("trie_search.bf16", o)
    assert o["operand_dtype"] == 1, o
    assert o["kernel"]["ok"], o["kernel"]["why"]
    _check(o["micro"], alone=8 * ROW_ALONE_ABS)


def test_eval_ddp_search_terms(dev, tmp_path):
    """--allowed_terms FILE --search_terms 8 --search_top 3 on synthetic:c1_tiny (the fake tokenizer): no generation, ranked_terms in
    --rank_terms' format; with 8 beams over 11 terms every search is exhaustive here, so the terms are --rank_terms' own."""
    import argparse
    import importlib.util
    from opus_pllm_amd import synth
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    terms = ["GO 0005634 nucleus", "GO 0005634 nuclear lumen", "GO 0005886 plasma membrane", "GO 0005886 membrane raft",
             "GO 0016020 membrane", "GO 0005737 cytoplasm", "GO 0005737", "EC 3.4.21.4", "EC 3.4.21.5", "EC 2.7.11.1", "kinase"]
    tfile, inp = tmp_path / "terms.txt", tmp_path / "q.json"
    tfile.write_text("\n".join(terms) + "\n")
    qs = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(40 + 9 * i, i), output="x") for i in range(3)]
    json.dump(qs, open(inp, "w"))

    def run(out, **kw):
        base = dict(model_base_path="synthetic:c1_tiny", opus_pllm_weights_path="synthetic", input_path=str(inp), save_path=str(out),
                    temperature=0.0, top_p=0.7, num_beams=1, max_new_tokens=6, switch_projector_type="mlp2x_gelu", load_4bit=False,
                    load_8bit=False, batch_size=2, max_residues=128, max_prompt=None, collective_timeout=60, use_input_embed=False,
                    stop_at_hashes=False, inflight=1, save_logprobs=False, dump_logits=None, allowed_terms=str(tfile),
                    allowed_separator=None, allowed_prefix="", rank_terms=0, rank_with_stop=False, search_terms=0, search_top=0)
        base.update(kw)
        ddp.eval_model(argparse.Namespace(**base))
        return json.load(open(out))

    got = run(tmp_path / "s.json", search_terms=8, search_top=3)
    want = run(tmp_path / "r.json", rank_terms=3)
    assert len(got) == 3 and all(len(r["ranked_terms"]) == 3 and r["generated"] == r["ranked_terms"][0][0] for r in got), got
    worst = 0.0
    for g, w in zip(got, want):
        assert all(t in terms for t, _ in g["ranked_terms"]) and all(a[1] >= b[1] for a, b in zip(g["ranked_terms"], g["ranked_terms"][1:]))
        lp = dict(w["ranked_terms"])
        for t, v in g["ranked_terms"]:
            if t in lp:
                worst = max(worst, abs(v - lp[t]))
    record("trie_search.search_terms", {"logprob_abs_vs_rank_terms": worst})
    with pytest.raises(ValueError, match="exclude"):
        run(tmp_path / "x.json", search_terms=8, rank_terms=3)
