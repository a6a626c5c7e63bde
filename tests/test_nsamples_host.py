"""Host tests (no GPU) of generate(num_return_sequences=N): the top-N result of the beam bookkeeping against the installed
transformers, the calls that raise, the trie a decoder row follows, the C ABI entries and the driver's flag."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from fake_tokenizer import FakeTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K,N,eos_mode", [(3, 1, "two"), (3, 2, "two"), (3, 3, "two"), (4, 4, "none"), (2, 2, "first"), (4, 3, "first3")])
def test_beam_top_n_matches_transformers(K, N, eos_mode):
    """beam.BeamState.result(N) / result_scores(N) against GenerationMixin._beam_search(num_return_sequences=N) of the local
    transformers on a tiny random CPU Llama (the pattern of test_host.py::test_beam_bookkeeping_matches_transformers): the N best
    finished hypotheses of every row, best first, cropped to the longest returned one; two EOS ids, rows finishing at different
    lengths, a row finishing at length 1."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from opus_pllm_amd.beam import BeamState
    torch.manual_seed(K * 7 + len(eos_mode))
    V, H, B, T, L, pad = 40, 32, 3, 5, 9, 0
    hf = LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=H, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                      num_key_value_heads=2, max_position_embeddings=64)).eval()
    with torch.no_grad():
        for prm in hf.parameters():
            prm.mul_(4.0)                                             # sharper distributions: beams diverge, EOS appears
    emb = torch.randn(B, T, H)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :2] = 0
    kw = dict(inputs_embeds=emb, attention_mask=mask, num_beams=K, do_sample=False, max_new_tokens=L, use_cache=True, pad_token_id=pad)
    with torch.no_grad():
        free = hf.generate(**kw, eos_token_id=None)
    eos = {"none": [], "two": [int(free[0, 2]), int(free[2, 4])], "first": [int(free[1, 0])],
           "first3": [int(free[0, 0]), int(free[1, 0]), int(free[2, 0])]}[eos_mode]
    with torch.no_grad():
        want = hf.generate(**kw, eos_token_id=eos or None, num_return_sequences=N, return_dict_in_generate=True, output_scores=True)

    st = BeamState(B, K, L, eos, pad, V)
    tok_emb = hf.get_input_embeddings()
    seqs = torch.zeros(B, K, 0, dtype=torch.long)
    while True:
        flat = seqs.reshape(B * K, -1)
        full = torch.cat([emb.repeat_interleave(K, 0), tok_emb(flat)], 1)
        fm = torch.cat([mask.repeat_interleave(K, 0), torch.ones(B * K, flat.shape[1], dtype=torch.long)], 1)
        pos = (fm.cumsum(-1) - 1).clamp(min=0)
        with torch.no_grad():
            lg = hf(inputs_embeds=full, attention_mask=fm, position_ids=pos).logits[:, -1].float()
        acc = torch.log_softmax(lg, -1).view(B, K, V) + torch.from_numpy(st.running_scores)[:, :, None]
        sc, ix = torch.topk(acc.view(B, K * V), st.M)
        tok, src, done = st.step(sc.numpy(), ix.numpy())
        if done:
            break
        seqs = torch.cat([seqs[torch.arange(B)[:, None], torch.from_numpy(src)], torch.from_numpy(tok)[:, :, None]], 2)
    got = st.result(N)
    assert got.shape == tuple(want.sequences.shape) and got.shape[0] == B * N, (got.shape, want.sequences.shape)
    assert np.array_equal(got, want.sequences.numpy()), (got, want.sequences)
    sc = st.result_scores(N)
    assert sc.shape == (B * N,)
    np.testing.assert_allclose(sc, want.sequences_scores.numpy(), rtol=1e-5, atol=1e-5)
    assert bool((np.diff(sc.reshape(B, N), axis=1) <= 0).all())      # best first
    assert np.array_equal(st.result(), st.result(1)) and np.array_equal(st.result(1)[:, : got.shape[1]], got[::N][:, : st.result(1).shape[1]])
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            st.result(bad)


def _bare(max_batch=8):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro(max_batch=max_batch)
    return m


def test_num_return_sequences_errors():
    """The four refusals, raised before anything touches the GPU, the first two with the messages of the reference's transformers 4.46.3."""
    from transformers import GenerationConfig
    m = _bare()
    ids = torch.ones((3, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        m.generate(ids, num_return_sequences=2, max_new_tokens=2)
    with pytest.raises(ValueError, match="without beam search do not support"):        # (the installed library words it likewise)
        GenerationConfig(num_return_sequences=2, do_sample=False).validate(strict=True)
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(4\) has to be smaller or equal to `num_beams` \(3\)"):
        m.generate(ids, num_beams=3, num_return_sequences=4, max_new_tokens=2)
    for kw in (dict(do_sample=True), dict(num_beams=2), {}):
        with pytest.raises(ValueError, match="num_return_sequences"):
            m.generate(ids, num_return_sequences=0, max_new_tokens=2, **kw)
    with pytest.raises(_cabi.OpusError, match="max_batch=8") as e:
        m.generate(ids, do_sample=True, num_return_sequences=3, max_new_tokens=2)       # 3 x 3 = 9 decoder rows
    assert e.value.code == -2


def test_decoder_row_follows_the_trie_of_its_prompt():
    """TokenTrie.per_row of B tries under num_return_sequences=N: row r follows trie r // N (repeat_interleave's layout); generate
    keeps asking for B tries, not B N."""
    from opus_pllm_amd.constraint import TokenTrie
    tries = [TokenTrie([[10 + b, 20 + b]], end_token_id=1) for b in range(3)]
    per_row = TokenTrie.per_row(tries)
    N = 5
    rows = torch.arange(3).repeat_interleave(N).tolist()
    for r, b in enumerate(rows):
        assert per_row.row_trie(r, N) is tries[b] and b == r // N
        assert per_row.row_trie(r, N).allowed_after([]) == [10 + b]
    assert [per_row.row_trie(r) for r in range(3)] == tries
    for r, n in ((15, N), (-1, N), (3, 1), (0, 0)):
        with pytest.raises(IndexError):
            per_row.row_trie(r, n)
    assert list(per_row.compiled().start.shape) == [3]                 # one start state per prompt: the kernel divides the row by N
    m = _bare(max_batch=16)
    with pytest.raises(ValueError, match="per_row"):                   # 15 tries for 3 prompts is refused as before
        m.generate(torch.ones((3, 4), dtype=torch.long), do_sample=True, num_return_sequences=N, max_new_tokens=2,
                   prefix_allowed_tokens_fn=TokenTrie.per_row([tries[0]] * 15))


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    for name, nargs in (("opus_llama_prefill_fanout", 8), ("opus_generate_scored_fanout", 19)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == nargs, (name, decl)
    # the existing entries keep their signatures, and the version does not move
    assert len(_cabi.SIGNATURES["opus_llama_prefill"][1]) == 7 and len(_cabi.SIGNATURES["opus_generate_scored"][1]) == 18
    assert re.search(r"#define\s+OPUS_ABI_VERSION\s+10\b", header) and _cabi.ABI_VERSION == 10
    if os.path.exists(_cabi.LIB_PATH):
        lib = _cabi.lib()
        assert lib.opus_abi_version() == 10
        assert hasattr(lib, "opus_llama_prefill_fanout") and hasattr(lib, "opus_generate_scored_fanout")


def _driver():
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flag_and_output_shape():
    ddp = _driver()
    p = ddp.build_parser()
    a = p.parse_args(["--input_path", "in.json", "--save_path", "out.json"])
    assert a.num_return_sequences == 1
    a = p.parse_args(["--input_path", "in.json", "--save_path", "out.json", "--num_return_sequences", "5", "--batch_size", "60"])
    assert a.num_return_sequences == 5 and ddp.prompts_per_call(a.batch_size, a.num_return_sequences) == 12
    assert ddp.prompts_per_call(8, 5) == 1 and ddp.prompts_per_call(8, 1) == 8
    with pytest.raises(ValueError):
        ddp.prompts_per_call(4, 5)
    qs = [{"output": "t0", "input": "A"}, {"output": "t1", "input": "C"}]
    one = ddp.build_result(qs, ["a", "b"])
    assert one == [{"ground_truth": "t0", "generated": "a"}, {"ground_truth": "t1", "generated": "b"}]      # N = 1: unchanged
    three = ddp.build_result(qs, ["a0", "a1", "a2", "b0", "b1", "b2"], 3)
    assert three == [{"ground_truth": "t0", "generated": "a0", "generated_all": ["a0", "a1", "a2"]},
                     {"ground_truth": "t1", "generated": "b0", "generated_all": ["b0", "b1", "b2"]}]
    with pytest.raises(ValueError):
        ddp.build_result(qs, ["a", "b", "c"], 2)


class _FakeModel:
    """Records what annotate() asks of generate() and answers with rows that name their prompt and sample."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def generate(self, ids, seqs, **kw):
        n = int(kw.get("num_return_sequences", 1))
        self.calls.append((ids.shape[0], list(seqs), n, kw.get("seed")))
        rows = [[100 + len(self.calls), 10 * b + j] for b in range(ids.shape[0]) for j in range(n)]
        return torch.tensor(rows, dtype=torch.long)


def test_driver_takes_batch_size_over_n_prompts_per_call():
    ddp = _driver()
    items = [{"instruction": f"what is <seq> number {i}", "input": "ACD" + "E" * i, "output": "x"} for i in range(7)]
    torch.manual_seed(0)
    m = _FakeModel()
    out = ddp.annotate(m, FakeTokenizer(), items, "data/any.json", 6, 4, temperature=0.1, num_return_sequences=3, device=m.device,
                       inflight=1)
    assert [c[0] for c in m.calls] == [2, 2, 2, 1] and all(c[2] == 3 for c in m.calls)      # 6 // 3 prompts per call
    assert [c[1] for c in m.calls][0] == [items[0]["input"], items[1]["input"]]
    assert out.shape == (7 * 3, 4)
    assert out[:, 1].tolist() == [10 * b + j for n in (2, 2, 2, 1) for b in range(n) for j in range(3)]   # item-major, samples inside
    m1 = _FakeModel()
    out1 = ddp.annotate(m1, FakeTokenizer(), items, "data/any.json", 6, 4, temperature=0.0, device=m1.device, inflight=1)
    assert [c[0] for c in m1.calls] == [6, 1] and all(c[2] == 1 for c in m1.calls) and out1.shape == (7, 4)
    with pytest.raises(ValueError):
        ddp.annotate(_FakeModel(), FakeTokenizer(), items, "data/any.json", 6, 4, num_return_sequences=0, device=m.device)
