"""search_trie() without a GPU: the CPU twin of the algorithm (tests/trie_search_ref.py) against the brute-force top-N of exact path
sums, the rules for narrow beams, ties, padding and members that are prefixes of other members; the search table; the refusals
OpusLlamaForCausalLM.search_trie raises before it touches the device; the C ABI's new symbols; eval_ddp.py's flags."""
import ctypes as C
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TRIE_MAX_DEPTH, TRIE_SEARCH_MAX_BEAMS, TokenTrie, TrieSearchTable
from opus_pllm_amd.model import OpusLlamaForCausalLM, OpusPrefix, TrieSearchResult
import trie_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("opus_set_trie_search", "opus_trie_search_begin", "opus_trie_search_level", "opus_debug_trie_beam_expand")
END = 1
F = np.float32


def random_trie(rng, n, lo=1, hi=5, alphabet=8, separator=None):
    members = [rng.integers(3, 3 + alphabet, int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]
    if n >= 2 and len(members[0]) > 1:
        members[1] = members[0][:-1]                                       # a member that is a prefix of another one
    return TokenTrie(members, END, separator=separator)


def tables(rng, trie, stop):
    """Seeded log-prob tables per trie node: node_lp < 0 (column 0, the root, 0) and stop terms < 0 (or None)."""
    n = trie.n_nodes + 1
    node = -rng.random(n).astype(F) * 4 - F(0.01)
    node[0] = 0
    return node, (-rng.random(n).astype(F) * 3 - F(0.01)) if stop else None


def widest_level(trie, stop):
    """The most candidates any level can offer: the nodes of a depth that compete for a slot."""
    by_depth = {}
    for v in range(1, trie.n_nodes + 1):
        if stop or trie.children[v]:
            by_depth[trie.node_depth[v]] = by_depth.get(trie.node_depth[v], 0) + 1
    return max(by_depth.values(), default=1)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------------ the table
def test_search_table_is_the_tries_children():
    rng = np.random.default_rng(3)
    a, b = random_trie(rng, 12, separator=[2, 30]), random_trie(rng, 5)
    tab = TrieSearchTable([a, b, a])
    assert tab.start.tolist() == [1, 1 + len(a.children), 1] and tab.trie_of_row.tolist() == [0, 1, 0]
    assert tab.n_states == 1 + len(a.children) + len(b.children) and tab.member[0] == -1 and tab.edge_off[1] == 0
    for k, t in enumerate((a, b)):
        root = int(tab.root[k])
        for n, kids in enumerate(t.children):
            e0, e1 = tab.edge_off[root + n], tab.edge_off[root + n + 1]
            assert tab.edge_tok[e0:e1].tolist() == sorted(kids)                        # the separator's edge is not part of it
            assert tab.edge_next[e0:e1].tolist() == [root + kids[x] for x in sorted(kids)]
            assert tab.stop_set[root + n] == k
        for m, node in enumerate(t.member_nodes):
            assert tab.member[root + node] == m
        assert (tab.member[root: root + len(t.children)] >= 0).sum() == len(t.member_ids)
        assert tab.stop_ids[tab.stop_off[k]: tab.stop_off[k + 1]].tolist() == t.stop_ids()
    assert tab.max_depth == max(a.max_depth, b.max_depth)


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_wide_beam_is_the_brute_force_topn(seed, stop):
    rng = np.random.default_rng(100 + seed)
    trie = random_trie(rng, int(rng.integers(3, 40)), hi=int(rng.integers(2, 7)))
    node, st = tables(rng, trie, stop)
    tab = TrieSearchTable([trie])
    K = widest_level(trie, stop)
    assert K <= 64
    for top in sorted({1, min(3, K), K}):
        got = ref.search(tab, 0, node, st, K, top)
        idx, tot, lp, sl = ref.brute_force(trie, node, st, top)
        assert got["exhaustive"] and same(got["member_index"], idx) and same(got["logprob"], tot) and same(got["member_logprob"], lp)
        if stop:
            assert same(got["stop_logprob"], sl)
        else:
            assert got["stop_logprob"] is None
        assert 1 <= got["levels"] <= trie.max_depth + (1 if stop else 0)


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_narrow_beam(seed, stop):
    rng = np.random.default_rng(200 + seed)
    trie = random_trie(rng, 60, lo=2, hi=6, alphabet=6)
    node, st = tables(rng, trie, stop)
    tab = TrieSearchTable([trie])
    assert widest_level(trie, stop) > 4
    everyone = ref.brute_force(trie, node, st, len(trie.member_ids))
    exact = dict(zip(everyone[0].tolist(), zip(everyone[1].tolist(), everyone[2].tolist(), everyone[3].tolist())))
    for K, top in ((1, 1), (2, 1), (2, 2), (4, 3)):
        got = ref.search(tab, 0, node, st, K, top)
        assert not got["exhaustive"]
        found = got["member_index"] >= 0
        n_found = int(found.sum())
        assert n_found >= 1 and found[:n_found].all() and (np.diff(got["logprob"][:n_found]) <= 0).all()       # sorted, padding last
        assert len(set(got["member_index"][found].tolist())) == int(found.sum())
        for m, tot, lp in zip(got["member_index"][found], got["logprob"][found], got["member_logprob"][found]):
            assert F(exact[int(m)][0]) == tot and F(exact[int(m)][1]) == lp                  # the exact path sum of that member
        assert (got["logprob"][~found] == -np.inf).all() and (got["member_logprob"][~found] == -np.inf).all()
        # pruning is exact: what the run without it returns, the run with it returns too
        free = ref.search(tab, 0, node, st, K, top, prune=False)
        assert same(free["member_index"], got["member_index"]) and same(free["logprob"], got["logprob"])
        assert free["levels"] >= got["levels"]


def test_pruning_stops_early_and_keeps_ties():
    # two members below one id each; the first level already fills the pool with -1 and the deep branch starts at -2: stop
    trie = TokenTrie([[3], [4, 5, 6, 7]], END)
    tab = TrieSearchTable([trie])
    node = np.zeros(trie.n_nodes + 1, F)
    node[trie.children[0][3]], node[trie.children[0][4]] = -1, -2
    got = ref.search(tab, 0, node, None, 2, 1)
    assert got["levels"] == 1 and got["member_index"].tolist() == [0] and got["exhaustive"]
    # a beam that TIES the top-th pool entry goes on (strictly below stops): member 1 ends at -1 as well and loses the tie by index
    node[trie.children[0][4]] = -1
    got = ref.search(tab, 0, node, None, 2, 1)
    assert got["levels"] == 4 and got["member_index"].tolist() == [0] and got["logprob"].tolist() == [-1.0]
    trie2 = TokenTrie([[4, 5, 6, 7], [3]], END)                                          # the deep member has the lower index: it wins
    tab2 = TrieSearchTable([trie2])
    node2 = np.zeros(trie2.n_nodes + 1, F)
    node2[trie2.children[0][3]], node2[trie2.children[0][4]] = -1, -1
    got = ref.search(tab2, 0, node2, None, 2, 1)
    assert got["levels"] == 4 and got["member_index"].tolist() == [0] and got["logprob"].tolist() == [-1.0]


def test_beam_ties_go_to_the_lower_beam_then_id():
    # four leaves-with-children of equal score below two parents; K = 3 keeps (beam 0, id 5), (beam 0, id 6), (beam 1, id 5)
    trie = TokenTrie([[3, 5, 9], [3, 6, 9], [4, 5, 9], [4, 6, 9]], END)
    tab = TrieSearchTable([trie])
    node = np.full(trie.n_nodes + 1, -1, F)
    node[0] = 0
    root = int(tab.start[0])
    beams = [(root + trie.children[0][3], F(-1)), (root + trie.children[0][4], F(-1)), (0, F(-np.inf))]
    new, pool, live, exh, tok, par, elp, _ = ref.expand_level(tab, beams, [], True, True, lambda k, e: node[tab.edge_next[e] - root],
                                                              None, 3, 1, False)
    assert (tok, par) == ([5, 6, 5], [0, 0, 1]) and [a for _, a in new] == [-2, -2, -2] and live and not exh and pool == []
    # dead and surplus rows: state 0, -inf, a valid id, their own row
    new, _, live, exh, tok, par, elp, _ = ref.expand_level(tab, beams[:1], [], True, True, lambda k, e: node[tab.edge_next[e] - root],
                                                           None, 3, 1, False)
    assert [s for s, _ in new][2] == 0 and new[2][1] == -np.inf and tok[2] == 0 and par[2] == 2 and elp[2] == -np.inf and exh


def test_padding_when_fewer_members_than_top():
    trie = TokenTrie([[3, 4], [3, 5]], END)
    tab = TrieSearchTable([trie])
    node = np.asarray([0, -1, -2, -3], F)
    for st in (None, np.asarray([0, -9, -1, -0.5], F)):
        got = ref.search(tab, 0, node, st, 4, 4)
        assert got["member_index"].tolist()[2:] == [-1, -1] and sorted(got["member_index"].tolist()[:2]) == [0, 1]
        assert (got["logprob"][2:] == -np.inf).all() and (got["member_logprob"][2:] == -np.inf).all() and got["exhaustive"]
        if st is not None:
            assert (got["stop_logprob"][2:] == -np.inf).all() and np.isfinite(got["stop_logprob"][:2]).all()
        assert not np.isnan(got["logprob"]).any()


def test_members_that_are_prefixes_of_members():
    # "3" is a member and a prefix of "3 4"; "3 4" of "3 4 5"
    trie = TokenTrie([[3], [3, 4], [3, 4, 5]], END)
    tab = TrieSearchTable([trie])
    n1, n2, n3 = trie.member_nodes
    node = np.zeros(4, F)
    node[n1], node[n2], node[n3] = -1, -0.5, -0.25
    got = ref.search(tab, 0, node, None, 1, 3)               # without a stop term: shorter is never worse
    assert got["member_index"].tolist() == [0, 1, 2] and got["logprob"].tolist() == [-1.0, -1.5, -1.75]
    assert got["levels"] == 3 and got["exhaustive"]
    #   ... the member "3" goes to the pool at level 1 AND its node keeps a beam (it has a child); the leaf "3 4 5" takes no slot
    assert [len(lv) for lv in got["trace"]] == [1, 1, 0]
    stop = np.zeros(4, F)
    stop[n1], stop[n2], stop[n3] = -5, -0.125, -3
    got = ref.search(tab, 0, node, stop, 1, 3)               # with it: the stop term is added one level later, from the beam's logits
    assert got["member_index"].tolist() == [1, 2, 0] and got["logprob"].tolist() == [-1.625, -4.75, -6.0]
    assert got["stop_logprob"].tolist() == [-0.125, -3.0, -5.0] and got["levels"] == 4 and [len(lv) for lv in got["trace"]] == [1, 1, 1, 0]
    got = ref.search(tab, 0, node, stop, 1, 1)               # top 1: stops once the beam (-1.75) is below the pool's -1.625
    assert got["member_index"].tolist() == [1] and got["levels"] == 3


# ------------------------------------------------------------------------------------------------ the refusals
def _hostless_model(**cap):
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro(**cap)
    return m


def test_refusals_before_the_device_is_touched():
    m = _hostless_model()
    cfg = m.cfg
    pre = OpusPrefix(m, 1, torch.zeros((2, cfg.dec_dim)), torch.tensor([10, 12]), slots=12)
    trie = TokenTrie([[3, 4], [3, 5]], END)
    with pytest.raises(TypeError):
        m.search_trie("prefix", trie)
    with pytest.raises(TypeError):
        m.search_trie(pre, [[3, 4]])
    with pytest.raises(ValueError, match="per_row"):
        m.search_trie(pre, TokenTrie.per_row([trie] * 3))
    for kw in (dict(top=0), dict(num_beams=0, top=0), dict(num_beams=2, top=3), dict(num_beams=TRIE_SEARCH_MAX_BEAMS + 1, top=1)):
        with pytest.raises(ValueError, match="top <= num_beams <= 16"):
            m.search_trie(pre, trie, **kw)
    assert cfg.max_new_tokens < TRIE_MAX_DEPTH
    with pytest.raises(ValueError, match="TRIE_MAX_DEPTH"):
        m.search_trie(pre, TokenTrie([[3] * (TRIE_MAX_DEPTH + 1)], END))
    with pytest.raises(ValueError, match=f"max_new_tokens={cfg.max_new_tokens}"):
        m.search_trie(pre, TokenTrie([[3] * (cfg.max_new_tokens + 1)], END))
    small = _hostless_model(max_batch=4)
    with pytest.raises(ValueError, match="max_batch>=8"):
        small.search_trie(OpusPrefix(small, 1, torch.zeros((2, cfg.dec_dim)), torch.tensor([10, 12]), slots=12), trie, num_beams=8)
    with pytest.raises(ValueError, match="max_prompt"):
        m.search_trie(OpusPrefix(m, 1, torch.zeros((2, cfg.dec_dim)), torch.tensor([10, 12]), slots=cfg.max_prompt), trie)
    with pytest.raises(ValueError, match="trie ids"):
        m.search_trie(pre, TokenTrie([[3, cfg.dec_vocab]], END))
    # generate() goes on refusing beams over a trie
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(torch.ones((2, 4), dtype=torch.long), num_beams=2, max_new_tokens=2, prefix_allowed_tokens_fn=trie)


def test_result_class():
    r = TrieSearchResult(torch.tensor([[1, -1]]), torch.tensor([[-1.0, float("-inf")]]), torch.tensor([[-0.5, float("-inf")]]), 3, 24,
                         torch.tensor([True]), torch.tensor([2]))
    assert r.logprob.tolist() == [[-1.5, float("-inf")]] and not torch.isnan(r.logprob).any()
    assert (r.levels, r.rows_decoded, r.trace) == (3, 24, None)
    r = TrieSearchResult(torch.tensor([[1]]), torch.tensor([[-1.0]]), None, 1, 0, torch.tensor([True]), torch.tensor([2]))
    assert r.logprob is r.member_logprob and r.stop_logprob is None


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_new_symbols_exported_and_bound(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    for name in NEW:
        assert name in _cabi.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.opus_abi_version() == _cabi.ABI_VERSION                          # additions: the version stays
    assert "typedef struct opus_trie_search_io" in header
    # the ctypes mirror lists the header's fields in order
    body = header.split("typedef struct opus_trie_search_io {")[1].split("}")[0]
    names = [w.strip(" *;") for line in body.splitlines() for w in line.split("/*")[0].replace(";", ",").split(",")]
    names = [n.split()[-1].lstrip("*") for n in names if n.strip()]
    assert names == [f for f, _ in _cabi.CTrieSearchIO._fields_], names


def test_argument_checks_return_before_any_hip_call():
    lib = _cabi.lib()
    assert lib.opus_set_trie_search(None, 2, None, None, None, 1, None, None, 1, None, None, None) == -1
    assert lib.opus_trie_search_begin(None, None, 1, None) == -1
    assert lib.opus_trie_search_level(None, None, 1, None) == -1
    assert lib.opus_debug_trie_beam_expand(None, None, 8, None, 1, None) == -1
    buf = C.create_string_buffer(512)
    _cabi.check(lib.opus_timing_names(buf, 512))
    classes = buf.value.decode().split(";")[0].split(",")
    assert "trie_search" in classes and classes[-3:] == ["mlm", "logitproc", "xent"]


def test_build_checks_the_new_kernels_for_scratch():
    spec = importlib.util.spec_from_file_location("opus_build", os.path.join(ROOT, "opus-pllm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "trie_search.hip" in b.SOURCES
    for kernel in ("trie_beam_expand_kernel", "trie_search_summary_kernel"):
        assert any(k in kernel for k in b.NO_SCRATCH), kernel


# ------------------------------------------------------------------------------------------------ the driver
def _ddp():
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    return ddp


def test_eval_ddp_flags(capsys):
    p = _ddp().build_parser()
    base = ["--input_path", "a.json", "--save_path", "b.json", "--allowed_terms", "t.txt"]
    a = p.parse_args(base + ["--search_terms", "8", "--search_top", "5", "--rank_with_stop"])
    assert (a.search_terms, a.search_top, a.rank_terms, a.rank_with_stop) == (8, 5, 0, True)
    a = p.parse_args(base + ["--rank_terms", "3"])
    assert (a.search_terms, a.search_top, a.rank_terms) == (0, 0, 3)
    with pytest.raises(SystemExit) as e:
        p.parse_args(base + ["--search_terms", "8", "--rank_terms", "3"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
