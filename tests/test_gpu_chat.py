"""Conversations on the GPU: generate(return_prefix=True) and the ragged export behind it (opus_llama_prefix_export_rows, bit for
bit against the rectangular export), a follow-up turn through the handle against plain generate() on the concatenated
conversation, cache_prefix(prefix=) (seal and rank, extend), ChatSession, the Llama-3-8B widths and the bf16 build
(tests/bf16_chat_check.py).  Every generated answer is forced by a one-member TokenTrie per row (tests/chat_checks.py), so ids
never depend on a margin and every (row, step) pair is compared.  Bounds are the project's own for the same effects (DESIGN.md
section 3); observed figures go through gpu_helpers.record."""
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import chat_checks as cc
import forward_checks as fc
import gen_scores_checks as gsc
import prefix_generate_checks as pg
from gpu_helpers import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO_REL_L2 = 1.5e-2          # behind a prefix vs plain on micro models (tests/test_gpu_prefix_generate.py), decode vs prefill
#                                (tests/test_gpu_parity.py): both effects are present in a turn behind a decoded history
DECODE_VS_PREFILL = 1.5e-2     # token_logprobs vs score_continuations (tests/test_gpu_prefix_generate.py)
ROW_VS_BATCH_LOGITS = 3e-3     # Llama-3-8B widths, a PREFILLED history behind a prefix vs plain (tests/test_gpu_prefix_generate.py)
# Llama-3-8B widths, a DECODED history (K / V the decode steps wrote) vs plain.  Not yet measured on an MI355X: until it is, the
# bound is ROW_VS_BATCH_LOGITS - the same kind of effect (the history's K / V projected by the decode step's GEMM route, M = rows,
# instead of the prefill's, M = rows x positions: the same fp16 operands, fp32 accumulation in another order) on the same rows.
# The convention of tests/test_gpu_batch64.py (3 x the observed figure) applies once test_llama3_8b_widths... has recorded one.
CHAT_WIDE_LOGITS = 3e-3
BF16_FACTOR = 8                # bf16 has 8 significand bits against fp16's 11 (tests/test_gpu_bf16.py)
PRESETS = {"micro": lambda: opa.micro(), "micro_qwen": lambda: opa.micro_qwen(), "micro_opt": lambda: opa.micro_opt(),
           "c1_tiny": lambda: opa.c1_tiny(max_prompt=128)}
EXPORT_OK = ("windows", "pads_zero", "kstart", "lengths_sum", "twice", "wider", "nonzero", "handle_same_bits")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fc.make_model(PRESETS[name](), dev)
        return cache[name]
    return get


def _assert_export(o):
    for part in ("plain", "behind"):
        assert all(o[part][k] for k in EXPORT_OK), (part, o[part])
    p = o["plain"]
    assert p["pending"] and p["lengths"] and p["context_unchanged"] and p["works_after_refusals"], p
    assert p["refusal_codes"] == [-2] * 5, p


# ------------------------------------------------------------------------------------------------ 1. the export kernel
@pytest.mark.parametrize("preset", ["micro", "micro_qwen", "micro_opt"])
def test_export_rows_bit_exact(models, preset):
    o = cc.export_checks(models(preset), seed=11)
    record(f"chat.export.{preset}", o)
    _assert_export(o)
    assert o["plain"]["keep"] == [1, 4, 7, 7] and o["plain"]["Tp"] == 21, o["plain"]       # the ragged ends are the chosen ones


def test_export_rows_window_crosses_slot_64(models):
    o = cc.export_checks(models("c1_tiny"), seed=12, plens=(60, 70, 33, 64))
    record("chat.export.c1_tiny_slot64", o)
    _assert_export(o)
    assert o["plain"]["crosses_64"] and o["plain"]["T0"] == 70, o["plain"]


def test_export_rows_needs_a_prefill(dev):
    model = fc.make_model(opa.micro(), dev)
    with pytest.raises(_cabi.OpusError) as e:
        model.export_cache_rows([0], 4)
    assert e.value.code == -6


# ------------------------------------------------------------------------------------------------ 2. turn 2 = the concatenation
@pytest.mark.parametrize("preset", ["micro", "micro_qwen", "micro_opt", "c1_tiny"])
def test_turns_equal_the_concatenated_conversation(models, preset):
    o = cc.turns_vs_concat(models(preset), seed=21)
    record(f"chat.turns.{preset}", o)
    assert o["ids_forced"] and o["new_context_bitwise"] and o["handle_unchanged"], o
    for t in ("turn2", "turn3"):
        assert o[t]["ids_equal"] and o[t]["rel_l2"] < MICRO_REL_L2 and o[t]["teacher_forced_abs"] < DECODE_VS_PREFILL, (t, o)


# ------------------------------------------------------------------------------------------------ 3. seal and rank
@pytest.mark.parametrize("preset", ["micro", "micro_opt"])
def test_seal_rank_and_extend(models, preset):
    o = cc.seal_and_rank(models(preset), seed=31)
    record(f"chat.seal.{preset}", o)
    assert o["sealed_is_live"] and o["extended_lengths"] and o["extend_ids_equal"], o
    assert o["rank_abs"] < DECODE_VS_PREFILL and o["extend_rel_l2"] < MICRO_REL_L2, o


def test_pending_handle_errors(models):
    model = models("micro")
    prompts, out, _ = cc.turn1(model, seed=32)
    h = out.prefix
    assert h.detached and h.pending is not None and h.pending.dtype == torch.int64
    with pytest.raises(ValueError, match=r"pending.*seal it with cache_prefix\(prefix=handle\)"):
        model.score_continuations(h, [[5, 6]] * 4)
    ids = torch.full((4, model.cfg.max_prompt - h.slots), 5)            # + the pending id: one position too many
    with pytest.raises(_cabi.OpusError, match=rf"max_prompt={model.cfg.max_prompt}.*max_prompt >= {model.cfg.max_prompt + 1}") as e:
        model.generate(ids, prefix=h, pad_token_id=cc.PAD, max_new_tokens=2)
    assert e.value.code == -2
    plain = model.cache_prefix(*_padded(prompts), detach=True)
    with pytest.raises(ValueError, match="row 0 is empty"):
        model.cache_prefix(torch.zeros((4, 0), dtype=torch.long), prefix=plain)
    out = model.generate(torch.zeros((4, 0), dtype=torch.long), prefix=h, pad_token_id=cc.PAD, eos_token_id=[], max_new_tokens=2)
    assert out.shape == (4, 2)                                           # an empty follow-up: the pending ids alone are fed


def _padded(rows):
    ids, mask = pg.left_pad(rows)
    return ids, None, mask


# ------------------------------------------------------------------------------------------------ 4. ChatSession
def test_chat_session(models):
    o = cc.session(models("micro"), seed=41)
    record("chat.session", o)
    assert o["ids_equal"] and o["logits_bitwise"] and o["turns"] == 3 and o["lengths"] and o["handle_bytes"] > 0, o
    assert o["rewind_bitwise"] and o["rewind_past_kept"] == "refused" and o["sampling_repeats"] and o["sampling_turns"] == 3, o


# ------------------------------------------------------------------------------------------------ 5. Llama-3-8B widths
def test_llama3_8b_widths_turn_behind_a_decoded_history(dev):
    model = fc.make_model(gsc.llama8b_shape(4, 2, 8), dev)
    o = cc.widths(model, seed=51)
    record("chat.llama_widths", o)
    del model
    torch.cuda.empty_cache()
    assert o["ids_equal"], o
    assert o["prefilled_history_rel_l2"] < ROW_VS_BATCH_LOGITS, o
    assert o["decoded_history_rel_l2"] < CHAT_WIDE_LOGITS, o


# ------------------------------------------------------------------------------------------------ 6. bf16
def test_bf16_build_chat():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_chat_check.py")], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_CHAT ")][-1]
    o = json.loads(line[len("BF16_CHAT "):])
    record("chat.bf16", o)
    assert o["operand_dtype"] == 1, o
    _assert_export(o["export"])
    t = o["turns"]
    assert t["ids_forced"] and t["new_context_bitwise"] and t["handle_unchanged"], t
    for k in ("turn2", "turn3"):
        assert t[k]["ids_equal"] and t[k]["rel_l2"] < BF16_FACTOR * MICRO_REL_L2, (k, t)
        assert t[k]["teacher_forced_abs"] < BF16_FACTOR * DECODE_VS_PREFILL, (k, t)
