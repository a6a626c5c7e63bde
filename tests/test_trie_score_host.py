"""Host-side parts of trie scoring (OpusLlamaForCausalLM.score_trie) that need no GPU: the member numbering of TokenTrie, the pass
plan of constraint.plan_trie_score (order, passes, re-computed chains, edges, stop rows, row counts), a numpy walk of the plan
over made-up logits against the flat sum of log-softmaxes, TrieScores.topk, the errors raised before any native call and the C
ABI additions of both library builds."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TRIE_MAX_DEPTH, TokenTrie, plan_trie_score
from opus_pllm_amd.model import OpusLlamaForCausalLM, OpusPrefix, TrieScores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("opus_llama_score_tree", "opus_llama_score_tree_scratch_bytes", "opus_llama_dec_rows_cap", "opus_llama_tree_max_depth",
       "opus_trie_path_sums", "opus_debug_attn_tree")
END = 1


def random_members(rng, n, vocab=12, lo=1, hi=6, with_prefix_members=True):
    """n id lists over a small alphabet (so that they share prefixes); some are prefixes of others, some repeat."""
    out = [rng.integers(3, 3 + vocab, int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]
    if with_prefix_members and n >= 4:
        out[1] = out[0][: max(1, len(out[0]) - 1)]                       # a member that is a prefix of another one
        out[3] = list(out[2])                                            # a duplicate
    return out


def shaped_trie(fan, seed=0, vocab=4000):
    """The vocabulary of fan-outs `fan` from seeded random ids (distinct among siblings)."""
    rng = np.random.default_rng(seed)
    paths = [[]]
    for f in fan:
        paths = [p + [int(t)] for p in paths for t in rng.choice(np.arange(3, vocab), size=f, replace=False)]
    return TokenTrie(paths, end_token_id=END)


CASES = {
    "single": lambda rng: [TokenTrie(random_members(rng, 40), END)] * 3,
    "separator": lambda rng: [TokenTrie(random_members(rng, 25, with_prefix_members=False), END, separator=[2, 30])] * 2,
    "per_row": lambda rng: [TokenTrie(random_members(rng, int(n)), END) for n in (5, 30, 1, 12)],
    "one_member": lambda rng: [TokenTrie([[7]], END)] * 2,
    "one_long_member": lambda rng: [TokenTrie([list(range(3, 3 + TRIE_MAX_DEPTH))], END)],
    "depth_limit": lambda rng: [TokenTrie(random_members(rng, 20, lo=TRIE_MAX_DEPTH - 3, hi=TRIE_MAX_DEPTH, vocab=2), END)] * 2,
}


def check_plan(tries, include_stop, cap):
    plan = plan_trie_score(tries, include_stop, cap)
    P, N = plan.P, plan.N
    assert P == len(tries) and N == max(t.n_nodes for t in tries) and plan.M == max(len(t.member_ids) for t in tries)
    want_eval = [[v for v in range(1, t.n_nodes + 1) if include_stop or t.children[v]] for t in tries]
    assert plan.evaluated_nodes == sum(len(w) for w in want_eval)
    scored_seq = [[] for _ in tries]                 # the scored rows of every prefix row, in plan order
    edge_slots, stop_slots = [], []
    extra = 0
    for ps in plan.passes:
        assert 0 <= ps.rows <= cap
        first_scored = int(np.argmax(ps.scored)) if ps.rows else 0
        assert not ps.scored[:first_scored].any() and ps.scored[first_scored:].all()     # the chain, then the run
        extra += first_scored
        for r in range(ps.rows):
            p, v, t = int(ps.prow[r]), int(ps.node[r]), tries[int(ps.prow[r])]
            assert ps.tok[r] == t.node_tok[v] and ps.depth[r] == t.node_depth[v]
            if t.node_par[v] == 0:
                assert ps.parent[r] == -1
            else:                                     # every parent in the pass (the run or the re-computed chain), earlier
                q = int(ps.parent[r])
                assert 0 <= q < r and ps.prow[q] == p and ps.node[q] == t.node_par[v]
            if ps.scored[r]:
                scored_seq[p].append(v)
            else:
                assert r < first_scored and (r == 0 or ps.parent[r] == r - 1)            # one chain, root to leaf
        if first_scored:
            assert ps.parent[first_scored] == first_scored - 1                             # ... of the pass's first node
        assert (np.diff(ps.edge_row) >= 0).all() and (np.diff(ps.stop_row) >= 0).all()
        for k, src in enumerate(ps.score_src):
            assert -P <= src < ps.rows and (src < 0 or ps.scored[src])                    # a re-computed row is never scored
            assert (ps.edge_row == k).any() or (ps.stop_row == k).any()                   # the lm_head only where it is used
        assert len(set(ps.score_src.tolist())) == len(ps.score_src)                       # once per scoring row
        for e in range(len(ps.edge_row)):
            src = int(ps.score_src[ps.edge_row[e]])
            p, child = divmod(int(ps.edge_slot[e]), N + 1)
            t = tries[p]
            u = 0 if src < 0 else int(ps.node[src])
            assert (src < 0 and -src - 1 == p) or ps.prow[src] == p
            assert t.children[u][int(ps.edge_tok[e])] == child
            edge_slots.append((p, child))
        for k in range(len(ps.stop_row)):
            src = int(ps.score_src[ps.stop_row[k]])
            p, v = divmod(int(ps.stop_slot[k]), N + 1)
            assert src >= 0 and ps.prow[src] == p and ps.node[src] == v and plan.tries[ps.stop_set[k]] is tries[p]
            stop_slots.append((p, v))
    for p, t in enumerate(tries):                     # preorder, children in ascending id; every evaluated node exactly once
        assert scored_seq[p] == [v for v in t.preorder().tolist() if include_stop or t.children[v]]
        assert sorted(scored_seq[p]) == want_eval[p]
    pre = tries[0].preorder().tolist()
    assert sorted(pre) == list(range(1, tries[0].n_nodes + 1))
    pos = {v: i for i, v in enumerate(pre)}
    for v in pre:                                     # (preorder: a parent precedes its children, siblings ascend by id)
        par = tries[0].node_par[v]
        assert par == 0 or pos[par] < pos[v]
    assert sorted(edge_slots) == [(p, v) for p, t in enumerate(tries) for v in range(1, t.n_nodes + 1)]
    want_stop = [(p, v) for p, t in enumerate(tries) for v in range(1, t.n_nodes + 1) if t.complete[v]] if include_stop else []
    assert sorted(stop_slots) == want_stop
    assert plan.rows_evaluated == plan.evaluated_nodes + extra
    return plan, extra


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("include_stop", [False, True])
def test_plan_invariants(case, include_stop):
    tries = CASES[case](np.random.default_rng(sorted(CASES).index(case)))
    plan, extra = check_plan(tries, include_stop, 10 ** 6)
    assert extra == 0 and len(plan.passes) == 1                                           # one pass: exactly the counts
    assert plan.rows_evaluated == sum(sum(1 for v in range(1, t.n_nodes + 1) if include_stop or t.children[v]) for t in tries)
    deepest = max(t.max_depth for t in tries)
    for cap in (deepest, deepest + 3, 100):
        plan, extra = check_plan(tries, include_stop, cap)
        assert all(ps.rows <= cap for ps in plan.passes)


def test_go_shaped_vocabulary_counts():
    t = shaped_trie((1, 1, 10, 20, 10))
    assert len(t.member_ids) == 2000 and t.n_nodes == 2212
    assert plan_trie_score([t] * 16, False, 10 ** 6).rows_evaluated == 3392
    assert plan_trie_score([t] * 16, True, 10 ** 6).rows_evaluated == 35392
    for chunk in (7, 100, 1000):
        plan, extra = check_plan([t], True, chunk)
        assert len(plan.passes) >= -(-2212 // chunk) and extra <= 4 * len(plan.passes)


def test_too_deep_or_no_room():
    deep = TokenTrie([list(range(3, 4 + TRIE_MAX_DEPTH))], END)
    with pytest.raises(ValueError):
        plan_trie_score([deep], False, 1000)
    with pytest.raises(ValueError):
        plan_trie_score([TokenTrie([[3, 4, 5, 6]], END)], True, 3)
    with pytest.raises(TypeError):
        plan_trie_score([object()], True, 10)


def test_member_numbering_brute_force():
    rng = np.random.default_rng(5)
    seqs = random_members(rng, 60, vocab=3, hi=4)                                         # many duplicates
    t = TokenTrie(seqs, END)
    distinct = []
    for s in seqs:
        if s not in distinct:
            distinct.append(s)
    assert len(distinct) < len(seqs)
    assert t.member_ids == distinct
    assert t.input_member == [distinct.index(s) for s in seqs]
    for ids, node in zip(t.member_ids, t.member_nodes):
        v = 0
        for tok in ids:
            v = t.children[v][tok]
        assert v == node and t.complete[v] and t.node_depth[v] == len(ids)
        path = []
        while v:
            path.append(t.node_tok[v])
            v = t.node_par[v]
        assert path[::-1] == ids
    assert t.member_strings is None

    class Tok:
        def encode(self, text, add_special_tokens=False):
            return [3 + (ord(c) % 7) for c in text.strip()]                               # ("ab" and "ab " are one member)

    strings = ["ab", "abc", "ab ", "b", "abc", "h"]                                       # ("h" encodes as "a": 104 % 7 == 97 % 7)
    ts = TokenTrie.from_strings(Tok(), strings, end_token_id=END)
    enc = [Tok().encode(x) for x in strings]
    dist = []
    for e in enc:
        if e not in dist:
            dist.append(e)
    assert ts.member_ids == dist and ts.input_member == [dist.index(e) for e in enc]
    assert ts.member_strings == [strings[[dist.index(e) for e in enc].index(m)] for m in range(len(dist))]
    assert ts.member_strings[0] == "ab" and len(ts.member_strings) == len(dist)


def fake_logits(p, path, V):
    return np.random.default_rng([p, len(path)] + list(path)).normal(size=V) * 3


def log_softmax(x):
    x = x - x.max()
    return x - np.log(np.exp(x).sum())


def walk(plan, tries, V):
    """What the native side does with a plan, in numpy: every scoring row's logits come from ITS path as the pass's parent links
    spell it."""
    P, N, M = plan.P, plan.N, plan.M
    node_lp = np.zeros((P, N + 1))
    stop_node = np.full((P, N + 1), -np.inf)
    for ps in plan.passes:
        lsm = []
        for src in ps.score_src:
            if src < 0:
                p, path = -int(src) - 1, []
            else:
                p, path, r = int(ps.prow[src]), [], int(src)
                while r >= 0:
                    path.append(int(ps.tok[r]))
                    r = int(ps.parent[r])
                path = path[::-1]
                assert len(path) == ps.depth[src]
            lsm.append(log_softmax(fake_logits(p, path, V)))
        for e in range(len(ps.edge_row)):
            node_lp.flat[ps.edge_slot[e]] = lsm[ps.edge_row[e]][ps.edge_tok[e]]
        for k in range(len(ps.stop_row)):
            ids = plan.stop_ids[plan.stop_off[ps.stop_set[k]]: plan.stop_off[ps.stop_set[k] + 1]]
            stop_node.flat[ps.stop_slot[k]] = np.log(np.exp(lsm[ps.stop_row[k]][ids]).sum())
    member = np.full((P, M), -np.inf)
    stop = np.full((P, M), -np.inf)
    for p in range(P):
        k = plan.trie_of_row[p]
        for m in range(M):
            v = plan.member_node[k, m]
            if v < 0:
                continue
            stop[p, m] = stop_node[p, v]
            path = []
            while v:
                path.append(v)
                v = plan.node_par[k, v]
            assert len(path) == plan.node_depth[k, path[0]]
            member[p, m] = sum(node_lp[p, u] for u in path[::-1])
    return node_lp, member, stop


@pytest.mark.parametrize("case", ["single", "separator", "per_row", "one_member"])
@pytest.mark.parametrize("cap", [10 ** 6, 9])
def test_numpy_walk_of_the_plan_matches_the_flat_sums(case, cap):
    V = 40
    tries = CASES[case](np.random.default_rng(100 + sorted(CASES).index(case)))
    plan = plan_trie_score(tries, True, cap)
    node_lp, member, stop = walk(plan, tries, V)
    for p, t in enumerate(tries):
        for m, ids in enumerate(t.member_ids):
            flat = sum(log_softmax(fake_logits(p, ids[:j], V))[ids[j]] for j in range(len(ids)))
            assert abs(member[p, m] - flat) < 1e-9
            want = np.log(np.exp(log_softmax(fake_logits(p, ids, V)))[t.stop_ids()].sum())
            assert abs(stop[p, m] - want) < 1e-9
        assert (member[p, len(t.member_ids):] == -np.inf).all() and (node_lp[p, t.n_nodes + 1:] == 0).all()
    assert tries[0].stop_ids() == [END] + ([2] if tries[0].separator else [])
    plan0 = plan_trie_score(tries, False, cap)
    node0, member0, _ = walk(plan0, tries, V)
    assert np.array_equal(node0, node_lp) and np.array_equal(member0, member)


def test_topk_matches_torch_and_breaks_ties_low():
    g = torch.Generator().manual_seed(3)
    lp = torch.randn(5, 37, generator=g)
    lp[2, 30:] = float("-inf")
    res = TrieScores(lp, None, torch.zeros(5, 50), torch.full((5,), 37), 0)
    assert res.logprob is lp
    for k in (1, 4, 37):
        v, i = res.topk(k)
        tv, ti = torch.topk(lp, k, dim=1)
        assert torch.equal(v, tv) and torch.equal(lp.gather(1, i), tv)
    tie = torch.tensor([[0.5, 2.0, 2.0, -1.0, 2.0]])
    v, i = TrieScores(tie, None, torch.zeros(1, 6), torch.tensor([5]), 0).topk(4)
    assert i.tolist() == [[1, 2, 4, 0]] and v.tolist() == [[2.0, 2.0, 2.0, 0.5]]
    with_stop = TrieScores(tie, tie * 2, torch.zeros(1, 6), torch.tensor([5]), 0)
    assert torch.equal(with_stop.logprob, tie * 3)
    with pytest.raises(ValueError):
        res.topk(38)


def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    return m


def test_errors_before_any_native_call():
    m = _hostless_model()
    cfg = m.cfg
    pre = OpusPrefix(m, 1, torch.zeros((2, cfg.dec_dim)), torch.tensor([10, 12]))
    trie = TokenTrie([[3, 4], [3, 5]], END)
    with pytest.raises(TypeError):
        m.score_trie("prefix", trie)
    with pytest.raises(TypeError):
        m.score_trie(pre, [[3, 4]])
    with pytest.raises(TypeError):
        m.score_trie(pre, lambda b, s: [3])
    with pytest.raises(ValueError):
        m.score_trie(pre, TokenTrie.per_row([trie, trie, trie]))
    with pytest.raises(ValueError):
        m.score_trie(pre, TokenTrie([[3, cfg.dec_vocab]], END))
    with pytest.raises(_cabi.OpusError) as e:
        m.score_trie(pre, TokenTrie([[3] * (TRIE_MAX_DEPTH + 1)], END))
    assert e.value.code == -2
    room = cfg.max_prompt + cfg.max_new_tokens
    long_pre = OpusPrefix(m, 1, torch.zeros((2, cfg.dec_dim)), torch.tensor([10, room - 1]))
    with pytest.raises(_cabi.OpusError) as e:
        m.score_trie(long_pre, trie)                                                      # row 1: room - 1 + 2 positions
    assert e.value.code == -2
    assert TRIE_MAX_DEPTH >= 32


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


def test_row_capacity_depth_limit_and_scratch():
    lib = _cabi.lib()
    assert lib.opus_abi_version() == 10
    assert lib.opus_llama_tree_max_depth() == TRIE_MAX_DEPTH
    micro = opa.micro(max_batch=2, max_prompt=40)
    mc = _cabi.CConfig.from_config(micro)
    assert lib.opus_llama_dec_rows_cap(C.byref(mc)) == 80
    big = _cabi.CConfig.from_config(opa.llama3_8b(max_batch=16, max_enc_tokens=66, max_prompt=110, max_new_tokens=16))
    assert lib.opus_llama_dec_rows_cap(C.byref(big)) == 16 * 110
    bad = _cabi.CConfig.from_config(micro)
    bad.dec_heads = 0
    assert lib.opus_llama_dec_rows_cap(C.byref(bad)) == -1
    a = lib.opus_llama_score_tree_scratch_bytes(C.byref(mc), 80, 82, 200, 40, 2, 1)
    b = lib.opus_llama_score_tree_scratch_bytes(C.byref(mc), 80, 82, 400, 40, 2, 1)
    assert 0 < a <= b and a % 256 == 0
    assert lib.opus_llama_score_tree_scratch_bytes(C.byref(mc), 0, 2, 2, 0, 0, 0) > 0      # (a pass of root edges alone)
    assert lib.opus_llama_score_tree_scratch_bytes(C.byref(mc), 81, 82, 200, 40, 2, 1) == -1
    assert lib.opus_llama_score_tree_scratch_bytes(C.byref(mc), 8, -1, 0, 0, 0, 0) == -1
    # the workspace of a context does not grow with the feature: the tables and slabs are caller scratch
    assert lib.opus_workspace_bytes(C.byref(mc)) > 0
    # argument checks that return before any HIP call
    assert lib.opus_llama_score_tree(None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, None, None, None, 0, None, 0,
                                     None, None, 1, 0, None, None, 1, None, 0, None) != 0
    assert lib.opus_debug_attn_tree(None, None, None, None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.opus_trie_path_sums(None, None, None, None, None, None, 1, 1, 2, None, None) == -1
