"""Host-side parts of conversations (generate(return_prefix=True), cache_prefix(prefix=), ChatSession, the drivers) that need no
GPU: the window arithmetic of the ragged export, where rows end, the pending id in front of a suffix, the refusals that return
before any device call, the Conversation deltas, the multi-turn driver loop on a stub model, and the C ABI additions."""
import argparse
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, conversation as conv_mod
from opus_pllm_amd.conversation import Conversation, SeparatorStyle
from opus_pllm_amd.constraint import TokenTrie
from opus_pllm_amd.model import OpusLlamaForCausalLM, OpusPrefix, _suffix_rows, counted_tokens
from opus_pllm_amd.prefix import plan_export_rows, snapshot_bytes
from fake_tokenizer import FakeTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"opus_llama_prefix_export_rows": 8, "opus_llama_prefix_behind": 11}


# ------------------------------------------------------------------------------------------------ plan_export_rows
def _brute(kstart, T0, keep):
    """slot by slot: which live slots belong to row r, and where they land in a snapshot as wide as the longest window"""
    live = [[s for s in range(T0 + max(keep)) if kstart[r] <= s < T0 + keep[r]] for r in range(len(kstart))]
    Tp = max(len(w) for w in live)
    return [len(w) for w in live], Tp, [Tp - len(w) for w in live]


@pytest.mark.parametrize("kstart,T0,keep", [
    ([5, 0, 9, 0], 14, [1, 4, 7, 7]),           # ragged padding and ragged ends
    ([5, 0, 9], 14, [0, 0, 0]),                 # nothing decoded is kept: the prompts alone
    ([0], 7, [3]),                              # a single row
    ([3], 4, [0]),                              # one real token, nothing kept
    ([0, 13], 14, [0, 9]),                      # the shortest prompt keeps the most
])
def test_plan_export_rows_named_cases(kstart, T0, keep):
    lengths, Tp, nks = plan_export_rows(kstart, T0, keep)
    want_len, want_Tp, want_nks = _brute(kstart, T0, keep)
    assert lengths.tolist() == want_len and Tp == want_Tp == max(want_len) and nks.tolist() == want_nks
    assert (nks + lengths == Tp).all() and nks.dtype == np.int32 and nks.min() == 0


def test_plan_export_rows_random_and_bad_input():
    rng = np.random.default_rng(3)
    for _ in range(200):
        R, T0 = int(rng.integers(1, 9)), int(rng.integers(1, 80))
        kstart, keep = rng.integers(0, T0, R).tolist(), rng.integers(0, 20, R).tolist()
        lengths, Tp, nks = plan_export_rows(kstart, T0, keep)
        assert (lengths.tolist(), Tp, nks.tolist()) == _brute(kstart, T0, keep)
    for bad in (([0, 1], 4, [1]), ([4], 4, [0]), ([-1], 4, [0]), ([0], 4, [-1]), ([], 4, []), ([0], 0, [0])):
        with pytest.raises(ValueError):
            plan_export_rows(*bad)


def test_handle_cost_is_snapshot_bytes():
    # Llama-3-8B: 32 layers x 8 kv heads x 128 x 2 bytes x (K and V) = 131 072 bytes per slot and row
    assert snapshot_bytes(32, 8, 128, 1, 1) == 131072
    h = OpusPrefix._snapshot(None, torch.zeros((2, 3, 2, 5, 16), dtype=torch.float16), torch.zeros((2, 3, 2, 5, 16), dtype=torch.float16),
                             torch.zeros(3, dtype=torch.int32), [0, 1, 2], torch.tensor([5, 4, 3]), 5, torch.tensor([7, 8, 9]))
    assert h.detached and h.rows == 3 and h.slots == 5 and h.nbytes() == snapshot_bytes(2, 2, 16, 3, 5) and h.pending.tolist() == [7, 8, 9]


# ------------------------------------------------------------------------------------------------ where rows end
def test_row_ends_with_pad_equal_to_eos_stop_sequence_and_no_end():
    eos = 2
    ids = torch.tensor([[7, 2, 2, 2, 2, 2],      # EOS at step 1, then pad == eos
                        [7, 8, 9, 2, 2, 2],      # EOS at step 3
                        [2, 2, 2, 2, 2, 2],      # EOS first: one id
                        [7, 8, 9, 4, 5, 6]])     # never ends
    n = counted_tokens(ids, [eos])
    assert n.tolist() == [2, 4, 1, 6]
    # keep = n - 1 decode slots, pending = the last counted id
    assert ids.gather(1, (n - 1).view(-1, 1)).view(-1).tolist() == [2, 2, 2, 6]
    stop = [9, 4]
    ids = torch.tensor([[7, 9, 4, 0, 0, 0], [9, 4, 0, 0, 0, 0], [7, 8, 9, 9, 9, 4], [4, 9, 7, 4, 9, 7], [7, 9, 2, 0, 0, 0]])
    assert counted_tokens(ids, [eos], stop).tolist() == [3, 2, 6, 6, 3]          # the stop sequence's last id counts; else EOS; else all
    assert counted_tokens(ids, [], stop).tolist() == [3, 2, 6, 6, 6]


# ------------------------------------------------------------------------------------------------ the pending id in front
def test_pending_id_goes_in_front_and_makes_an_empty_row_legal():
    ids = torch.tensor([[0, 5, 6], [0, 0, 0], [7, 8, 9]])
    mask = torch.tensor([[0, 1, 1], [0, 0, 0], [1, 1, 1]]).bool()
    pend = types.SimpleNamespace(rows=3, pending=torch.tensor([40, 41, 42]))
    rows, src = _suffix_rows(pend, None, ids, mask)
    assert [r.tolist() for r in rows] == [[40, 5, 6], [41], [42, 7, 8, 9]] and src.tolist() == [0, 1, 2]
    rows, src = _suffix_rows(pend, [2, 2, 0], ids, mask)                         # the pending id of the row each suffix continues
    assert [r.tolist() for r in rows] == [[42, 5, 6], [42], [40, 7, 8, 9]]
    rows, _ = _suffix_rows(pend, None, torch.zeros((3, 0), dtype=torch.long), None)      # sealing: no suffix at all
    assert [r.tolist() for r in rows] == [[40], [41], [42]]
    plain = types.SimpleNamespace(rows=3, pending=None)
    with pytest.raises(ValueError, match="row 1 is empty"):
        _suffix_rows(plain, None, ids, mask)
    rows, _ = _suffix_rows(plain, None, ids[[0, 2, 2]], mask[[0, 2, 2]])
    assert [r.tolist() for r in rows] == [[5, 6], [7, 8, 9], [7, 8, 9]]
    with pytest.raises(ValueError, match="prefix_rows must lie in"):
        _suffix_rows(pend, [0, 1, 3], ids, mask)
    with pytest.raises(ValueError, match="pass prefix_rows"):
        _suffix_rows(pend, None, ids[:2], mask[:2])


# ------------------------------------------------------------------------------------------------ refusals before the device
def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    m._stop_ids = []
    return m


@pytest.mark.parametrize("kw,word", [(dict(num_beams=2), "num_beams"), (dict(num_return_sequences=2, do_sample=True, seed=1), "num_return_sequences"),
                                     (dict(guidance_scale=1.5), "guidance_scale"),
                                     (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens")])
def test_return_prefix_refuses_what_is_not_built(kw, word):
    m = _hostless_model()
    with pytest.raises(NotImplementedError) as e:
        m.generate(torch.ones((1, 4), dtype=torch.long), max_new_tokens=2, return_dict_in_generate=True, return_prefix=True, **kw)
    assert "return_prefix" in str(e.value) and word in str(e.value)


def test_return_prefix_needs_return_dict():
    m = _hostless_model()
    with pytest.raises(ValueError, match="return_prefix.*return_dict_in_generate"):
        m.generate(torch.ones((1, 4), dtype=torch.long), max_new_tokens=2, return_prefix=True)


def test_scoring_refuses_a_pending_handle():
    m = _hostless_model()
    cfg = m.cfg
    z = torch.zeros((cfg.dec_layers, 2, cfg.dec_kv_heads, 12, cfg.dec_head_dim), dtype=torch.float16)
    h = OpusPrefix._snapshot(m, z, z.clone(), torch.zeros(2, dtype=torch.int32), [0, 2], torch.tensor([12, 10]), 12, torch.tensor([5, 6]))
    trie = TokenTrie([[3, 4], [3, 5]], 1)
    for call in (lambda: m.score_continuations(h, [[3, 4], [5]]), lambda: m.score_trie(h, trie), lambda: m.search_trie(h, trie)):
        with pytest.raises(ValueError, match=r"pending.*: seal it with cache_prefix\(prefix=handle\)"):
            call()


# ------------------------------------------------------------------------------------------------ Conversation deltas
def _styles():
    sys_ = "A chat."
    return {
        "single": dict(system=sys_, roles=["Student", "Professor"], sep_style=SeparatorStyle.SINGLE, sep="###"),
        "two": dict(system=sys_, roles=["USER", "ASSISTANT"], sep_style=SeparatorStyle.TWO, sep=" ", sep2="</s>"),
        "mpt": dict(system="<|im_start|>system\nS", roles=["<|im_start|>user\n", "<|im_start|>assistant\n"], sep_style=SeparatorStyle.MPT,
                    sep="<|im_end|>"),
        "llama2": dict(system=sys_, roles=["USER", "ASSISTANT"], sep_style=SeparatorStyle.LLAMA_2, sep="<s>", sep2="</s>"),
        "plain": dict(system="", roles=["", ""], sep_style=SeparatorStyle.PLAIN, sep="\n", sep2="</s>"),
    }


def _delta_property(c: Conversation):
    users, replies = ["What is <seq>?", "Which domain does that?", "Give the GO terms."], ["It binds ATP.", "The kinase domain."]
    c.append_message(c.roles[0], users[0])
    c.append_message(c.roles[1], None)
    text = c.get_prompt()                                     # the first turn's prompt, up to the assistant cue
    for u, a in zip(users[1:], replies):
        c.messages[-1]["content"] = a
        text += c.answer_segment(a) + c.turn_delta(u)
        c.append_message(c.roles[0], u)
        c.append_message(c.roles[1], None)
        assert c.get_prompt() == text, (c.sep_style, c.get_prompt(), text)
    return text


@pytest.mark.parametrize("style", list(_styles()))
def test_conversation_delta_property_for_every_self_rendered_style(style):
    text = _delta_property(Conversation(messages=[], offset=0, **_styles()[style]))
    assert "Which domain does that?" in text and "The kinase domain." in text


def test_conversation_delta_presets_and_errors():
    for preset in (conv_mod.conv_vicuna_v0, conv_mod.conv_vicuna_v1, conv_mod.conv_vicuna_v2, conv_mod.conv_vicuna_v3):
        _delta_property(preset.copy())
    c = conv_mod.conv_vicuna_v0.copy()
    with pytest.raises(ValueError):
        c.turn_delta("q")                                     # no answer to continue
    c.append_message(c.roles[0], "q")
    c.append_message(c.roles[1], "a")
    with pytest.raises(ValueError):
        c.turn_delta("")
    for st in (SeparatorStyle.LLAMA_3, SeparatorStyle.Qwen_2):
        d = Conversation(system="", roles=["u", "a"], messages=[{"role": "u", "content": "q"}, {"role": "a", "content": "x"}], offset=0,
                         sep_style=st, sep="")
        with pytest.raises(NotImplementedError):
            d.turn_delta("next")


class _Template:
    """ChatML through apply_chat_template; `rewrite` makes the template change history (it numbers the turns in a header)."""

    def __init__(self, rewrite=False):
        self.rewrite = rewrite

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=False):
        head = f"[{len(messages)} messages]\n" if self.rewrite else ""
        out = head + "".join(f"<|im_start|>{m['role']}\n{m['content']}<|im_end|>\n" for m in messages)
        return out + ("<|im_start|>assistant\n" if add_generation_prompt else "")


def test_conversation_delta_through_a_chat_template():
    c = Conversation(system="", roles=["user", "assistant"], messages=[], offset=0, sep_style=SeparatorStyle.Qwen_2, sep="",
                     tokenizer=_Template())
    c.append_message("user", "What is it?")
    first = c.get_prompt_eval()
    c.append_message("assistant", "A kinase.")
    d = c.turn_delta("Which domain?")
    assert d == "<|im_end|>\n<|im_start|>user\nWhich domain?<|im_end|>\n<|im_start|>assistant\n"
    c.append_message("user", "Which domain?")
    assert c.get_prompt_eval() == first + c.answer_segment("A kinase.") + d
    c.tokenizer = _Template(rewrite=True)
    c.append_message("assistant", "The catalytic one.")
    with pytest.raises(ValueError, match="not render the conversation so far as a prefix"):
        c.turn_delta("And then?")


# ------------------------------------------------------------------------------------------------ ChatSession and the driver
class _StubModel:
    """generate() records its arguments and answers with fixed ids and a stand-in handle."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def generate(self, inputs, seq=None, **kw):
        self.calls.append(dict(kw, inputs=inputs, seq=seq))
        n = len(self.calls)
        out = types.SimpleNamespace(sequences=torch.tensor([[10 + n, 11 + n, 2]]), prefix=types.SimpleNamespace(
            name=f"h{n}", lengths=torch.tensor([inputs.shape[1] + 2 + (0 if kw.get("prefix") is None else int(kw["prefix"].lengths[0]) + 1)])))
        return out


def test_chat_session_on_a_stub_model():
    m = _StubModel()
    chat = opa.ChatSession(m)
    assert chat.prefix is None and chat.lengths is None and chat.turns == []
    a1 = chat.ask(torch.tensor([[1, 5, 6, 7]]), seq=["MKV"], max_new_tokens=4)
    assert m.calls[0]["return_prefix"] and m.calls[0]["return_dict_in_generate"] and "prefix" not in m.calls[0]
    assert m.calls[0]["seq"] == ["MKV"] and m.calls[0]["max_new_tokens"] == 4 and a1.prefix.name == "h1"
    ids = chat.ask(torch.tensor([[8, 9]]), return_dict_in_generate=False, do_sample=True)
    assert torch.equal(ids, torch.tensor([[12, 13, 2]]))            # as plain generate(): the ids
    assert m.calls[1]["prefix"].name == "h1" and m.calls[1]["do_sample"] and chat.prefix.name == "h2"
    assert chat.lengths.tolist() == [4 + 2 + 1 + 2 + 2] and len(chat.turns) == 2 and chat.turns[1][0].tolist() == [[8, 9]]
    chat.ask(torch.tensor([[3]]))
    assert m.calls[2]["prefix"].name == "h2"
    chat.rewind(1)
    assert chat.prefix.name == "h2" and len(chat.turns) == 2
    with pytest.raises(ValueError, match="keep_handles=True"):
        chat.rewind(1)                                              # h1 was dropped: the default keeps two
    with pytest.raises(ValueError):
        chat.rewind(5)
    with pytest.raises(ValueError):
        chat.ask(torch.tensor([[3]]), prefix=object())
    chat.reset()
    assert chat.prefix is None and chat.turns == []
    keep = opa.ChatSession(m, keep_handles=True)
    for _ in range(3):
        keep.ask(torch.tensor([[3]]))
    keep.rewind(2)
    assert len(keep.turns) == 1 and keep.prefix is not None


def _load_eval_online():
    spec = importlib.util.spec_from_file_location("eval_online", os.path.join(ROOT, "opus-pllm_amd", "eval_online.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_multi_turn_driver_loop_on_a_stub_model():
    online = _load_eval_online()
    tok = FakeTokenizer()
    tok.batch_decode = lambda ids, skip_special_tokens=True: ["a reply ### Student: more"] * len(ids)
    m = _StubModel()
    chat = opa.ChatSession(m)
    args = argparse.Namespace(temperature=0.0, top_p=1.0, max_new_tokens=8, repetition_penalty=None, no_repeat_ngram_size=None,
                              min_new_tokens=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)
    shown, seq, reply = online.chat_once(chat, tok, "What does it do?", "MKVL", args)
    assert seq == "MKVL" and shown.startswith(opa.DEFAULT_SEQ_TOKEN) and reply == "a reply"
    first = m.calls[0]
    assert "prefix" not in first and first["return_prefix"] and first["inputs"][0, 0] == tok.bos_token_id
    assert opa.DEFAULT_SEQ_TOKEN_INDEX in first["inputs"][0].tolist() and first["seq"] == "MKVL"
    assert first["stop_sequence"] == tok("###").input_ids[1:] and first["do_sample"] is False
    shown, seq, reply = online.chat_once(chat, tok, "Which domain does that?", "", args)
    second = m.calls[1]
    assert second["prefix"].name == "h1" and seq is None and second["seq"] is None
    assert tok.bos_token_id not in second["inputs"][0].tolist()                 # a continuation: no BOS in front
    # only what the turn adds: the separator line, the student's turn, the cue - not the system text or the first question
    assert second["inputs"][0].tolist() == tok("\n### Student: Which domain does that?\n### Professor:").input_ids[1:]
    assert second["inputs"].shape[1] < first["inputs"].shape[1]
    assert online.chat_once(chat, tok, " /new ", "", args) is None and chat.prefix is None and chat.turns == []
    online.chat_once(chat, tok, "Another protein?", "", args)
    assert "prefix" not in m.calls[2] and m.calls[2]["inputs"][0, 0] == tok.bos_token_id and len(m.calls) == 3


# ------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_new_symbols_exported_and_bound(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NEW.items():
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert lib.opus_abi_version() == _cabi.ABI_VERSION == 10            # additive: the version stays
    assert C.sizeof(_cabi.CPrefixSnap) == 4 * C.sizeof(C.c_void_p) + 8  # and so does struct opus_prefix_snap


def test_new_entries_refuse_null_arguments_before_any_device_call():
    lib = _cabi.lib()
    assert lib.opus_llama_prefix_export_rows(None, 1, None, 1, None, None, None, None) != 0
    assert lib.opus_llama_prefix_behind(None, None, None, 1, 1, None, None, None, None, None, None) != 0
