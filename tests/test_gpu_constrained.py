"""GPU tests of constrained decoding (generate(prefix_allowed_tokens_fn=TokenTrie)): the kernel against the CPU restatement
(tests/constrained_ref.py) bit for bit, the micro model against the reference's own constrained generate
(tests/golden/generate_constrained_micro.npz, tools/gen_golden_constrained.py), the Llama-3-8B shape at batch 64 for greedy and
sampling, graphs and the default path, early stop, two contexts, the multiple-choice driver, and the bf16 build.  Nothing here
reads the reference."""
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
import constrained_checks as cc
import gen_scores_checks as gsc
from gpu_helpers import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_L2 = 1.5e-2            # scores / logits vs the reference's fp32 (tests/test_gpu_logits_proc.py)
SELF_ABS = 1e-5            # token_logprobs vs fp64 log_softmax of the returned raw logits (tests/test_gpu_logits_proc.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def micro(dev):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    from opus_pllm_amd import synth
    cfg = opa.micro(max_batch=12)
    canon = synth.canonical_weights(cfg, 0)
    return OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, canon, dev), dev)


@pytest.fixture(scope="module")
def big(dev):
    return gsc.make_model(gsc.llama8b_shape(B=64, layers=2, max_new=16), dev)


def _check_kernel(res):
    assert len(res) >= 300
    for name, r in res.items():
        assert r["banned_equal"] and r["allowed_identical"] and r["state_equal"], (name, r)
    assert max(r["widest"] for r in res.values()) > 4096                  # a root with more than 4 096 children
    assert sum(r["in_end_state"] for r in res.values()) > 0
    for V in (96, 128256, 152064):
        for B in (1, 64):
            for L in (0, 1, 17, 255):
                assert any(k.startswith(f"V{V}_B{B}_") and f"_L{L}_" in k for k in res), (V, B, L)


def _check_big(res):
    for mode, r in res.items():
        assert r["rejected_rows"] == 0 and r["drawn_not_allowed"] == 0, (mode, r)
        assert r["lp_abs"] <= SELF_ABS, (mode, r)
        if mode.startswith("greedy"):
            assert r["argmax_mismatch"] == 0 and r["scores_mismatch"] == 0, (mode, r)
        else:
            assert r["scores_mismatch"] == r["mismatch_near_threshold"], (mode, r)
        assert r["differs_from_plain"] and r["widest_allowed"] > 4096, (mode, r)
    banned = set(res["greedy"]["first_ids"])                              # bad words of the _proc modes: never chosen there
    for mode, r in res.items():
        if mode.endswith("_proc"):
            assert not banned & set(r["first_ids"]), (mode, r["first_ids"], banned)


def test_kernel_matches_restatement(big, dev):
    """opus_debug_token_constraint at V 96 / 128 256 / 152 064, B 1 and 64, tables from one member to 50 000 members of up to 16
    ids (a root with more than 4 096 children), separators, per-row starts, histories of 0 / 1 / 17 / 255 ids that stay on the
    trie, leave it, end: -inf where the restatement has it, every other entry bit-identical, the state word = the host walk."""
    res = cc.kernel(big, dev)
    record("constrained.kernel", res)
    _check_kernel(res)


def test_micro_matches_reference_fixture(micro):
    """Every id of every case equals the reference's; the -inf pattern of the scores is equal; scores (finite part) and raw
    logits within REL_L2."""
    res = cc.golden(micro)
    record("constrained.golden", res)
    assert set(res) == {"shared", "per_row", "list", "shared_pen", "list_ngram"}
    for tag, r in res.items():
        assert r["ids_equal"], (tag, r)
        assert r["inf_pattern_equal"], (tag, r)
        assert r["scores_rel_l2"] < REL_L2 and r["logits_rel_l2"] < REL_L2, (tag, r)


def test_llama8b_shape_greedy_and_sampling(big, dev):
    """Batch 64, 16 steps, a 50 000-member table, the constraint alone and with every other processor on."""
    res = cc.big(big, dev, B=64, max_new=16)
    record("constrained.big", res)
    assert len(res) == 6
    _check_big(res)


def test_graphs_and_default_path(big, dev):
    res = cc.graphs(big, dev)
    record("constrained.graphs", res)
    assert res["plain_equal_fresh"] and res["plain_equal"] and res["plain_new_graphs"] == 0 and res["plain_replays"] > 0, res
    assert res["on_graphs_second"] == 0 and res["on_graphs_first"] <= 1, res   # another trie, other starts: the same graph
    assert res["on_changed_ids"] and res["second_changed_ids"] and res["first_on_trie"] and res["second_on_trie"], res
    assert res["timing_off_launches"] == 0 and res["timing_on_launches"] == 4, res
    assert res["all_launches_on"] == res["all_launches_off"] + 4, res          # exactly one more launch per step


def test_early_stop_under_a_constraint(micro):
    res = cc.early_stop(micro)
    record("constrained.early_stop", res)
    for k, r in res.items():
        assert r["ids_equal"] and r["n"] < 16 and r["decode_steps"] <= r["n"] + 2, (k, r)


def test_two_contexts_follow_their_own_tries(micro):
    res = cc.two_contexts(micro)
    record("constrained.two_contexts", res)
    assert res == {"shared": True, "per_row": True}, res


def test_eval_multichoice_constrained(dev, tmp_path):
    """--constrained on synthetic:c1_tiny: every item is answered with one of its own option texts, and a batch of 2 gives what
    two batches of 1 give."""
    import argparse
    import importlib.util
    from opus_pllm_amd import synth
    spec = importlib.util.spec_from_file_location("eval_multichoice", os.path.join(ROOT, "opus-pllm_amd", "eval_multichoice.py"))
    em = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(em)
    qs = [dict(question="Where is it located?", options=["A) nucleus", "B) membrane", "C) cytosol", "D) secreted"][: 4 - (i % 2) * 2],
               input=synth.synth_protein(40 + 9 * i, i) if i != 2 else "", answer="B) membrane") for i in range(4)]
    inp = tmp_path / "q.json"
    json.dump(qs, open(inp, "w"))
    got = {}
    for bs in (2, 1):
        out = tmp_path / f"o{bs}.json"
        args = argparse.Namespace(model_base_path="synthetic:c1_tiny", opus_pllm_weights_path="synthetic", input_path=str(inp),
                                  save_path=str(out), temperature=0.0, top_p=0.7, num_beams=1, max_new_tokens=12,
                                  switch_projector_type="mlp2x_gelu", load_4bit=False, load_8bit=False, batch_size=bs,
                                  max_residues=128, max_prompt=256, rank_options=False, constrained=True)
        em.eval_model(args)
        got[bs] = [r["generated"] for r in json.load(open(out))]
    record("constrained.multichoice", got)
    from opus_pllm_amd import builder, conversation
    tok = builder.SyntheticTokenizer(opa.c1_tiny().dec_vocab)             # (decodes ids as "<id> <id> ...")
    shown = {L: em.after_process_output(tok.batch_decode([em.option_ids(tok, L)])[0], conversation.conv_vicuna_v3) for L in "ABCD"}
    assert len(set(shown.values())) == 4
    for q, text in zip(qs, got[2]):
        assert text in [shown[L] for L in "ABCD"[: len(q["options"])]], (q["options"], text, shown)
    assert got[2] == got[1], got


def test_bf16_build_constrained():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_constrained_check.py")], capture_output=True, text=True,
                       env=env, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_CONSTRAINED ")][-1]
    o = json.loads(line[len("BF16_CONSTRAINED "):])
    record("constrained.bf16", o)
    assert o["operand_dtype"] == 1, o
    _check_kernel(o["kernel"])
    assert set(o["big"]) == {"greedy", "greedy_proc"}
    _check_big(o["big"])
