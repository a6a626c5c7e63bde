"""Prompt-lookup decoding without a GPU: the twin (tests/lookup_ref.py) against transformers' PromptLookupCandidateGenerator, the
sentinel rules, lockstep acceptance and commit against a per-row restatement, the whole loop against plain greedy search, and
the argument checks of generate(prompt_lookup_num_tokens=...)."""
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import LookupStats, OpusLlamaForCausalLM, _check_lookup, lookup_history
from opus_pllm_amd.prompt import add_lookup_args, lookup_kwargs
import lookup_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the draft rule
@pytest.mark.parametrize("k", [1, 3, 10])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_draft_twin_equals_transformers(k, m):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(num_output_tokens=k, max_matching_ngram_size=m, max_length=10 ** 6)
    rng = random.Random(100 * k + m)
    hits = 0
    for L in range(2, 41):
        for vocab in (4, 5, 6):
            h = [rng.randrange(vocab) for _ in range(L)]
            t = torch.tensor([h], dtype=torch.long)
            cand, _ = gen.get_candidates(t)
            want = cand[0, L:].tolist()
            assert LR.draft(h, k, m) == want, (h, k, m)
            hits += bool(want)
    assert hits > 60                                            # (matches abound: the comparison is not one of empty drafts)


def test_draft_sentinel_rules():
    # a window over a protein block never matches: "5 6" before the block and "5 6" at the end are separated by -1 inside
    assert LR.draft([5, -1, 6, 9, 5, -1, 6], 3, 2) == [9, 5]             # tail (-1, 6) is skipped, m = 1 matches "6"
    assert LR.draft([4, -1, 8, 4, -1], 3, 2) == []                        # the tail holds -1 at every m
    # the draft is cut in front of a block / the separator
    assert LR.draft([1, 2, 3, 9, -1, 1, 2], 5, 2) == [3, 9]
    assert LR.draft([1, 2, -1, 7, 1, 2], 5, 2) == []                      # the continuation begins with -1: no match there
    assert LR.draft([1, 2, -1, 7, 2, 5, 1, 2], 5, 2) == [5, 1, 2]         # ... so m = 1 finds the later "2"
    # corpus separator: prompt "7 8 9" | corpus "3 7 8"; generated so far: nothing.  The match is the prompt's, cut at the separator
    h = LR.history([7, 8, 9], None, [3, 7, 8])
    assert h == [7, 8, 9, -1, 3, 7, 8] and LR.draft(h, 5, 2) == [9]
    # a match that starts in the corpus continues into the generated ids
    assert LR.draft(LR.history([1], None, [4, 5, 6]) + [4, 5], 2, 2) == [6, 4]
    assert LR.draft([2], 3, 2) == [] and LR.draft([], 3, 2) == []
    assert LR.draft([3, 3, 3, 3], 2, 3) == [3]                            # first start wins: i = 0, continuation h[3:4]


def test_history_matches_the_package(gold):
    g = gold("generate_micro")
    rows, lens = lookup_history(torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), None, 4)
    for b in range(3):
        want = LR.history(g["ids"][b].tolist(), g["mask"][b].tolist(), None, n_prot_tokens=4)
        assert rows[b, :lens[b]].tolist() == want and -200 not in want and want.count(-1) == 4
    corpus = [[5, 6], [], [9, -1, 10]]
    rows, lens = lookup_history(torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), corpus, 1)
    for b in range(3):
        want = LR.history(g["ids"][b].tolist(), g["mask"][b].tolist(), [t for t in corpus[b] if t >= 0], n_prot_tokens=1)
        assert rows[b, :lens[b]].tolist() == want
    assert rows.dtype == np.int32 and (rows[0, lens[0]:] == -1).all()
    with pytest.raises(ValueError):
        lookup_history(torch.from_numpy(g["ids"]), None, [[1]], 1)


# ------------------------------------------------------------------------------------------------ acceptance and commit
def _copy(st):
    c = LR.State(len(st.ids), st.stride, st.pad)
    c.ids, c.fin, c.step, c.next, c.n_unf = [r[:] for r in st.ids], st.fin[:], st.step, st.next[:], st.n_unf[:]
    return c


def _same(a, b):
    return (a.ids, a.fin, a.step, a.next, a.n_unf) == (b.ids, b.fin, b.step, b.next, b.n_unf)


def test_commit_equals_the_per_row_restatement_on_crafted_cases(gold):
    import lookup_checks as LC
    seen = {}
    for name, st, x, y, dl, eos, stop in LC.commit_cases(gold("generate_micro")["free_ids"]):
        a, b = _copy(st), _copy(st)
        ra = LR.commit(a, x, y, dl, 1, eos, stop)
        rb = LR.commit_per_row(b, x, y, dl, 1, eos, stop)
        assert ra == rb and _same(a, b), name
        seen[name] = (ra[0], a)
    assert seen["accept_none"][0] == 0 and seen["accept_all"][0] == 4 and seen["partial"][0] == 2
    assert seen["rows_differ_min_rules"][0] == 1 and seen["short_draft_len_rules"][0] == 2
    a, st = seen["eos_accepted"]
    assert a == 5 and st.fin == [0, 1, 0] and st.ids[1][4] == 85 and st.ids[1][5:8] == [2, 2, 2] and st.ids[0][7] != 2
    a, st = seen["eos_rejected"]
    assert a == 1 and st.fin == [0, 0, 0] and st.step == 3
    a, st = seen["budget_inside_chain"]
    assert a == 2 and st.step == 11 and all(r[11] != 2 for r in st.ids)
    a, st = seen["finished_row_ignored"]
    assert a == 4 and st.ids[1][4:9] == [2] * 5 and st.fin[1] == 1
    a, st = seen["stop_sequence"]
    assert st.fin[0] == 1 and st.ids[0][6] == 2 and st.fin[1:] == [0, 0]


def test_commit_equals_the_per_row_restatement_on_random_passes():
    rng = random.Random(7)
    for trial in range(300):
        R, stride, n = rng.randrange(1, 5), rng.randrange(6, 14), rng.randrange(1, 7)
        st = LR.State(R, stride, 0)
        st.step = rng.randrange(0, stride - 1)
        st.fin = [int(rng.random() < 0.2) for _ in range(R)]
        for b in range(R):
            for c in range(st.step + 1):
                st.ids[b][c] = rng.randrange(1, 5)
        st.next = [st.ids[b][st.step] for b in range(R)]
        y = [[rng.randrange(1, 5) for _ in range(n)] for _ in range(R)]
        x = [[st.next[b]] + [y[b][j] if rng.random() < 0.7 else rng.randrange(1, 5) for j in range(n - 1)] for b in range(R)]
        dl = [rng.randrange(0, n) for _ in range(R)]
        eos = (4,) if trial % 2 else ()
        stop = (1, 2) if trial % 3 == 0 else ()
        pre = 1 if n > 1 or trial % 2 else 0
        a, b = _copy(st), _copy(st)
        assert LR.commit(a, x, y, dl, pre, eos, stop) == LR.commit_per_row(b, x, y, dl, pre, eos, stop), trial
        assert _same(a, b), trial
        assert a.step <= stride - 1


def _model_fn(seed, vocab, period):
    """A pure 'model': the next id depends on the last two ids and the row, and cycles often (drafts hit)."""
    def f(b, ids):
        a, c = (ids[-1] if ids else 0), (ids[-2] if len(ids) > 1 else 0)
        return (a * 7 + c * 3 + b + seed + (len(ids) // period)) % vocab + 1
    return f


@pytest.mark.parametrize("k", [1, 3, 7])
def test_lookup_loop_equals_plain_greedy_search(k):
    total = {"passes": 0, "accepted": 0}
    for seed in range(12):
        R, max_new = 1 + seed % 3, 9 + 5 * (seed % 4)
        f = _model_fn(seed, 5, 6)
        hists = [[(3 * b + j) % 5 + 1 for j in range(4 + b)] for b in range(R)]
        for eos, stop in (((), ()), ((3,), ()), ((), (2, 4)), ((5,), (1, 1))):
            plain = LR.generate_plain(f, R, max_new, eos, stop, pad=0)
            got, stats = LR.generate(f, hists, max_new, k, 2, eos, stop, pad=0)
            assert got == plain, (seed, eos, stop)
            n_tok = len(plain[0])
            assert stats["passes"] + stats["plain_steps"] <= max(n_tok - 1, 0)
            assert stats["accepted"] <= stats["drafted"]
            total["passes"] += stats["passes"]
            total["accepted"] += stats["accepted"]
    assert total["passes"] > 0 and total["accepted"] > 0


def test_stop_sequence_across_a_pass_border_and_eos_in_the_rejected_part():
    # the model emits 1 2 3 4 5 6 7 8 ...; the stop sequence (4, 5) has its first id committed by one pass, its second by the next
    f = lambda b, ids: len(ids) + 1                                       # noqa: E731
    hist = [[9, 1, 2, 3, 4, 8, 8]]                                        # drafts "2 3 4" behind 1, then the wrong "8 8" behind 4
    got, stats = LR.generate(f, hist, 12, 3, 1, (), (4, 5), pad=0)
    assert got == [[1, 2, 3, 4, 5]] and stats["passes"] >= 1 and stats["accepted"] == 3
    # an EOS id in the rejected part of a draft finishes nothing: history drafts "7" (the EOS) behind 1, the model says 2
    got, _ = LR.generate(f, [[1, 7, 7]], 6, 2, 1, (7,), (), pad=0)
    assert got == [[1, 2, 3, 4, 5, 6]]
    # the budget cuts a chain: 5 ids asked for, a draft of 4 right ids behind the first
    got, stats = LR.generate(f, [[1, 2, 3, 4, 5, 6, 7]], 4, 6, 1, (), (), pad=0)
    assert got == [[1, 2, 3, 4]] and stats["passes"] == 1 and stats["accepted"] == 2


# ------------------------------------------------------------------------------------------------ the public surface
def _hostless_model(**cfg_kw):
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro(**cfg_kw)
    m._stop_ids = []
    return m


@pytest.mark.parametrize("kw,word", [(dict(do_sample=True, seed=1), "do_sample"), (dict(num_beams=2), "num_beams"),
                                     (dict(guidance_scale=2.0), "guidance_scale"), (dict(prefix=object()), "prefix"),
                                     (dict(repetition_penalty=1.3), "logits processors"),
                                     (dict(no_repeat_ngram_size=2), "logits processors"),
                                     (dict(return_dict_in_generate=True, output_scores=True), "output_scores"),
                                     (dict(return_dict_in_generate=True, output_logits=True), "output_scores"),
                                     (dict(return_dict_in_generate=True, output_token_logprobs=True), "output_scores")])
def test_combinations_not_built_raise_with_a_reason(kw, word):
    m = _hostless_model(max_batch=16)
    ids = torch.ones((1, 4), dtype=torch.long)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3, **kw)
    assert word in str(e.value) and "greedy" in str(e.value)


def test_more_refusals_and_the_max_batch_error():
    from opus_pllm_amd.constraint import TokenTrie
    m = _hostless_model(max_batch=16)
    ids = torch.ones((2, 4), dtype=torch.long)
    with pytest.raises(NotImplementedError) as e:
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3, prefix_allowed_tokens_fn=TokenTrie([[5, 6]], end_token_id=3))
    assert "TokenTrie" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        _check_lookup(3, None, 1, 16, nret=2)
    assert "num_return_sequences" in str(e.value)
    with pytest.raises(ValueError) as e:                       # 2 x (7 + 1) = 16 fits, 2 x (8 + 1) = 18 does not
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=8)
    assert "max_batch >= 18" in str(e.value) and "max_batch=16" in str(e.value)
    assert _check_lookup(7, None, 2, 16) == 2 and _check_lookup(7, 3, 2, 16) == 3
    for bad in (0, 9):
        with pytest.raises(ValueError):
            _check_lookup(3, bad, 1, 16)
    with pytest.raises(ValueError):
        _check_lookup(-1, None, 1, 16)
    assert repr(LookupStats(1, 2, 3, 4)) == "LookupStats(passes=1, plain_steps=2, drafted=3, accepted=4)"


def test_driver_options():
    import argparse
    p = argparse.ArgumentParser()
    add_lookup_args(p)
    assert lookup_kwargs(p.parse_args([])) == {}
    assert lookup_kwargs(p.parse_args(["--prompt_lookup_num_tokens", "0"])) == {}
    assert lookup_kwargs(p.parse_args(["--prompt_lookup_num_tokens", "7"])) == {"prompt_lookup_num_tokens": 7}
    assert lookup_kwargs(p.parse_args(["--prompt_lookup_num_tokens", "7", "--max_matching_ngram_size", "3"])) == \
        {"prompt_lookup_num_tokens": 7, "max_matching_ngram_size": 3}
    for drv in ("eval_online.py", "eval_ddp.py"):
        src = open(os.path.join(ROOT, "opus-pllm_amd", drv)).read()
        assert "add_lookup_args(p)" in src and "lookup_kwargs(args)" in src, drv


def test_new_symbols_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name in ("opus_generate_lookup", "opus_llama_verify_step", "opus_debug_lookup_draft", "opus_debug_lookup_accept"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _cabi.SIGNATURES and hasattr(lib, name)
        n_args = len(re.search(name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1).split(","))
        assert n_args == len(_cabi.SIGNATURES[name][1]), name
    assert lib.opus_abi_version() == _cabi.ABI_VERSION            # additive: new symbols only, the version stays
    assert "lookup.hip" in open(os.path.join(ROOT, "opus-pllm_amd", "build.py")).read()
