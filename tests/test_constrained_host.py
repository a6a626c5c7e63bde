"""Host tests (no GPU) of constrained decoding: the TokenTrie callback against a brute-force definition, the compiled table
against the callback, the CPU restatement (tests/constrained_ref.py) against the installed transformers'
PrefixConstrainedLogitsProcessor, a small CPU LlamaForCausalLM generating under the callback, the fixture's own promises
(tests/golden/generate_constrained_micro.npz), the C ABI entries, and the calls that raise."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TokenTrie
from opus_pllm_amd.model import OpusLlamaForCausalLM
import constrained_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
END, PAD = [90, 91], 91


def _members(rng, n, vocab=40, longest=6):
    return [[int(t) for t in rng.integers(0, vocab, size=int(rng.integers(1, longest + 1)))] for _ in range(n)]


def _histories(rng, members, sep, vocab=40):
    """On the trie (every prefix of members and of lists of members), off it, behind an end id, behind pads."""
    out = [[]]
    for m in members[:6]:
        out += [m[:k] for k in range(1, len(m) + 1)]
        out.append(m + [END[0]])
        out.append(m + [END[1], PAD, PAD])
        out.append(m[:-1] + [int(rng.integers(0, vocab))])
        out.append(m + [int(rng.integers(0, vocab))])
        out.append([int(rng.integers(0, vocab))] + m)
        if sep is not None:
            other = members[int(rng.integers(0, len(members)))]
            for k in range(len(sep) + 1):
                out.append(m + sep[:k])
            out += [m + sep + other[:k] for k in range(1, len(other) + 1)]
            out.append(m + sep + other + sep + m)
            out.append(m + sep + other + [END[0], PAD])
            out.append(m + sep[:-1] + [END[0]]) if len(sep) > 1 else None
    out.append([PAD, PAD])
    return out


CASES = [(0, 1, None), (1, 5, None), (2, 30, None), (3, 30, [77]), (4, 12, [77, 78, 77]), (5, 200, [50, 51])]


@pytest.mark.parametrize("seed,n,sep", CASES)
def test_callback_matches_brute_force_and_table(seed, n, sep):
    """The callback equals a scan over all members for every history; the compiled CSR table, walked as the kernel walks it
    (binary search, state 0 on a miss), allows exactly the same ids."""
    rng = np.random.default_rng(seed)
    members = _members(rng, n)
    trie = TokenTrie(members, end_token_id=END, separator=sep)
    tab = trie.compiled()
    assert tab.edge_off[0] == 0 and tab.edge_off[1] == 0 and tab.completing[0] == 1 and tab.edge_off[-1] == tab.n_edges
    for s in range(tab.n_states):                                       # ascending ids within a state
        ids = tab.edge_tok[tab.edge_off[s]: tab.edge_off[s + 1]]
        assert (np.diff(ids) > 0).all()
    for h in _histories(rng, members, sep):
        want = cref.brute_allowed(members, END, sep, h)
        assert trie(0, h) == want, (h, trie(0, h), want)
        assert trie(3, torch.tensor(h, dtype=torch.long)) == want        # (a tensor, as transformers passes it; batch id ignored)
        assert tab.allowed(tab.walk(0, h)) == want, h
        assert len(want) >= 1


def test_per_row_callback_and_table():
    rng = np.random.default_rng(11)
    sets = [_members(rng, 8), _members(rng, 3), _members(rng, 20)]
    seps = [None, [77], None]
    tries = [TokenTrie(m, end_token_id=END, separator=s) for m, s in zip(sets, seps)]
    rows = TokenTrie.per_row([tries[0], tries[1], tries[2], tries[0]])      # (a trie shared by two rows is stored once)
    tab = rows.compiled()
    assert len(tab.start) == 4 and tab.start[0] == tab.start[3] and len(set(tab.start.tolist())) == 3
    assert tab.n_states == 1 + sum(t.compiled().n_states - 1 for t in tries)
    for b, k in enumerate((0, 1, 2, 0)):
        for h in _histories(rng, sets[k], seps[k]):
            want = cref.brute_allowed(sets[k], END, seps[k], h)
            assert rows(b, h) == want and tab.allowed(tab.walk(b, h)) == want, (b, h)
    assert rows.compiled() is tab and tries[0].compiled() is tries[0].compiled()      # compiled once


def test_go_sized_vocabulary_compiles():
    """50 000 members of up to 16 ids, a root with more than 4 096 children."""
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 17, size=50000)
    members = [np.concatenate([rng.integers(0, 6000, size=1), rng.integers(6000, 6064, size=n - 1)]).tolist() for n in lens]
    trie = TokenTrie(members, end_token_id=128001)
    tab = trie.compiled()
    root = int(tab.start[0])
    assert tab.edge_off[root + 1] - tab.edge_off[root] > 4096 and tab.n_states > 300000
    for m in members[:50]:
        s = tab.walk(0, m)
        assert s != 0 and tab.completing[s]
        assert tab.walk(0, m + [128001]) == 0


@pytest.mark.parametrize("t", [0, 1, 3, 7])
@pytest.mark.parametrize("sep", [None, [77]])
def test_restatement_matches_transformers(t, sep):
    pytest.importorskip("transformers")
    rng = np.random.default_rng(5 + t)
    members = _members(rng, 16)
    trie = TokenTrie(members, end_token_id=END, separator=sep)
    B, V = 6, 96
    hs = [h for h in _histories(rng, members, sep) if len(h) == t][:B]
    while len(hs) < B:
        hs.append([int(x) for x in rng.integers(0, 40, size=t)])
    hist = torch.tensor(hs, dtype=torch.long).reshape(B, t)
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(t)) * 3
    ours = cref.process(x, hist, trie)
    assert torch.equal(ours.view(torch.int32), cref.hf_process(x, hist, trie).view(torch.int32))
    assert torch.isinf(ours).sum() > 0 and torch.isfinite(ours).any(dim=1).all()
    import logits_proc_ref as lpr
    for pen, min_new in ((1.3, 0), (0.8, 5), (None, 5)):                # behind the penalty and min_new_tokens
        pre = lpr.process(x, hist, eos=END, penalty=pen, min_new=min_new)
        both = cref.process(pre, hist, trie)
        ref = cref.hf_process(x, hist, trie, penalty=pen, min_new=min_new, eos=END)
        assert torch.equal(both.view(torch.int32), ref.view(torch.int32)), (pen, min_new)


@pytest.mark.parametrize("sep", [None, [77]])
def test_cpu_llama_generates_members(sep):
    """transformers' own generate from inputs_embeds with the object as prefix_allowed_tokens_fn: every row is a member (or a
    separator-joined list of members) followed by the end id."""
    tf = pytest.importorskip("transformers")
    torch.manual_seed(3)
    cfg = tf.LlamaConfig(vocab_size=96, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=2, max_position_embeddings=128, pad_token_id=PAD, eos_token_id=END, bos_token_id=None)
    model = tf.LlamaForCausalLM(cfg).eval()
    rng = np.random.default_rng(9)
    members = _members(rng, 24)
    trie = TokenTrie(members, end_token_id=END, separator=sep)
    emb = torch.randn(4, 5, 32)
    for kw in (dict(do_sample=False), dict(do_sample=True, temperature=1.5, top_k=0)):
        out = model.generate(inputs_embeds=emb, attention_mask=torch.ones(4, 5, dtype=torch.long), max_new_tokens=40,
                             prefix_allowed_tokens_fn=trie, pad_token_id=PAD, eos_token_id=END, **kw)
        for row in out.tolist():
            if any(t in END for t in row):
                assert cref.accepted(members, END, sep, row, pad=PAD), row
            else:                                                       # (a list that never ended inside 40 ids: still on the trie)
                assert sep is not None and trie(0, row) != END, row


def test_build_time_errors():
    with pytest.raises(ValueError, match="empty member"):
        TokenTrie([[1, 2], []], end_token_id=9)
    with pytest.raises(ValueError, match="end id 9 inside the member"):
        TokenTrie([[1, 9, 2]], end_token_id=[8, 9])
    with pytest.raises(ValueError, match="end id inside the separator"):
        TokenTrie([[1, 2]], end_token_id=9, separator=[5, 9])
    with pytest.raises(ValueError, match="ambiguous separator"):
        TokenTrie([[1, 2], [1, 2, 5, 3]], end_token_id=9, separator=[5])
    with pytest.raises(ValueError, match="at least one member"):
        TokenTrie([], end_token_id=9)
    with pytest.raises(ValueError, match="end_token_id"):
        TokenTrie([[1]], end_token_id=None)
    with pytest.raises(ValueError, match="share their end ids"):
        TokenTrie.per_row([TokenTrie([[1]], end_token_id=9), TokenTrie([[1]], end_token_id=8)])
    t = TokenTrie([[1, 2], [1, 2], [1, 2, 3]], end_token_id=9)          # duplicates merge
    assert len(t.children) == 4 and t(0, [1, 2]) == [3, 9]
    assert TokenTrie([[1, 2], [1, 2, 3]], end_token_id=9, separator=[5])(0, [1, 2]) == [3, 5, 9]


def test_from_strings_uses_prefix_and_no_special_tokens():
    class Tok:
        eos_token_id = 1

        def encode(self, text, add_special_tokens=True):
            assert add_special_tokens is False
            return [10 + ord(c) % 50 for c in text]
    trie = TokenTrie.from_strings(Tok(), ["ab", "ac"], end_token_id=1, separator="; ", prefix=" ")
    sp, a, b = 10 + ord(" ") % 50, 10 + ord("a") % 50, 10 + ord("b") % 50
    assert trie(0, []) == [sp] and trie(0, [sp, a]) == sorted([b, 10 + ord("c") % 50])
    assert trie.separator == [10 + ord(";") % 50, sp]
    assert "space" in TokenTrie.from_strings.__doc__


def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    return m


def test_generate_refuses_what_is_not_built():
    m = _hostless_model()
    ids = torch.ones((2, 4), dtype=torch.long)
    trie = TokenTrie([[3, 4]], end_token_id=27)
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(ids, num_beams=2, max_new_tokens=2, prefix_allowed_tokens_fn=trie)
    with pytest.raises(NotImplementedError, match="TokenTrie"):
        m.generate(ids, max_new_tokens=2, prefix_allowed_tokens_fn=lambda b, s: [1])
    with pytest.raises(ValueError, match="per_row"):
        m.generate(ids, max_new_tokens=2, prefix_allowed_tokens_fn=TokenTrie.per_row([trie] * 3))
    with pytest.raises(ValueError, match="outside"):
        m.generate(ids, max_new_tokens=2, prefix_allowed_tokens_fn=TokenTrie([[3, 96]], end_token_id=27))
    with pytest.raises(ValueError, match="outside"):
        m.generate(ids, max_new_tokens=2, prefix_allowed_tokens_fn=TokenTrie([[3]], end_token_id=400))


def test_new_symbols_are_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name, nargs in (("opus_set_token_constraint", 12), ("opus_debug_token_constraint", 9)):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        fn = getattr(lib, name)
        assert fn.restype == ctypes.c_int and fn.argtypes == _cabi.SIGNATURES[name][1]
    assert lib.opus_abi_version() == 10
    bf = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    assert bf.opus_set_token_constraint is not None and bf.opus_debug_token_constraint is not None
    assert lib.opus_set_token_constraint(None, 0, None, None, None, 0, None, None, 0, None, 0, None) != 0     # null context
    buf = ctypes.create_string_buffer(512)
    _cabi.check(lib.opus_timing_names(buf, 512))
    classes = buf.value.decode().split(";")[0].split(",")
    assert "constraint" in classes and classes[-1] == "xent", classes


def test_fixture_keeps_its_promises():
    """Every contested step of the reference run has a processed top-1 margin of at least 0.10, each case has at least 3 of them,
    list_ngram differs from list; the restatement applied to the reference's raw logits (behind the other processors) gives its
    scores bit for bit and its ids; every finished row is accepted."""
    import logits_proc_ref as lpr
    gp = dict(np.load(os.path.join(GOLD, "generate_constrained_micro.npz")))
    end = int(gp["end"])
    tags = sorted({k.split(".")[0] for k in gp if "." in k})
    assert tags == ["list", "list_ngram", "per_row", "shared", "shared_pen"] and int(gp["N"]) == 16 and end == 27
    for tag in tags:
        spec, kw = json.loads(str(gp[tag + ".spec"])), json.loads(str(gp[tag + ".kw"]))
        tries = [TokenTrie(t["members"], end_token_id=end, separator=t["sep"]) for t in spec["tries"]]
        fn = TokenTrie.per_row(tries) if spec["per_row"] else tries[0]
        seq = torch.from_numpy(gp[tag + ".sequences"])
        sc, lg = torch.from_numpy(gp[tag + ".scores"]), torch.from_numpy(gp[tag + ".logits"])
        contested, worst = 0, float("inf")
        for t in range(seq.shape[1]):
            pre = lpr.process(lg[t], seq[:, :t], eos=[end], penalty=kw.get("repetition_penalty"), ngram=kw.get("no_repeat_ngram_size", 0))
            p = cref.process(pre, seq[:, :t], fn)
            assert torch.equal(p.view(torch.int32), sc[t].view(torch.int32)), (tag, t)
            fin = (seq[:, :t] == end).any(1)
            am = torch.from_numpy(np.argmax(p.numpy(), axis=1))
            assert torch.equal(am[~fin], seq[~fin, t]), (tag, t)
            for b in range(seq.shape[0]):
                if not fin[b] and len(fn(b, seq[b, :t])) > 1:
                    top = sc[t, b].topk(2).values
                    contested += 1
                    worst = min(worst, float(top[0] - top[1]))
        assert contested >= 3 and worst >= 0.10, (tag, contested, worst)
        assert contested == int(gp[tag + ".contested"])
        for b, row in enumerate(seq.tolist()):
            t = spec["tries"][b if spec["per_row"] else 0]
            if end in row:
                assert cref.accepted(t["members"], [end], t["sep"], row, pad=int(gp["pad"])), (tag, row)
    assert not np.array_equal(gp["list.sequences"], gp["list_ngram.sequences"])
    assert os.path.getsize(os.path.join(GOLD, "generate_constrained_micro.npz")) <= 153 * 1024
