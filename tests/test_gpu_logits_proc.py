"""GPU tests of generate()'s logits processors (repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length /
min_new_tokens): the kernel against the CPU restatement (tests/logits_proc_ref.py) bit for bit, the micro model against the
reference's own generate (tests/golden/generate_processors_micro.npz, tools/gen_golden_processors.py), the Llama-3-8B shape at
batch 64 for greedy and sampling, graphs and the default path, early stop, and the bf16 build.  Nothing here reads the
reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import gen_scores_checks as gsc
import logits_proc_checks as lpc
from gpu_helpers import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REL_L2 = 1.5e-2            # scores / logits vs the reference's fp32 (tests/test_gpu_gen_scores.py)
SELF_ABS = 1e-5            # token_logprobs vs fp64 log_softmax of the returned raw logits


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
    assert len(res) >= 50
    for name, r in res.items():
        assert r["bitwise"] and r["untouched_identical"], (name, r)
    assert sum(r["banned"] for r in res.values()) > 0 and sum(r["edited"] for r in res.values()) > 0


def _check_big(res, sampling=True):
    for mode, r in res.items():
        assert r["lp_abs"] <= SELF_ABS, (mode, r)
        if mode.startswith("greedy"):
            assert r["argmax_mismatch"] == 0 and r["scores_mismatch"] == 0, (mode, r)
        else:
            assert r["scores_mismatch"] == r["mismatch_near_threshold"], (mode, r)
            assert r["drawn_not_finite"] == 0, (mode, r)
    assert res["greedy_p08"]["edited_chosen"] >= 1, res["greedy_p08"]
    assert res["greedy"]["differs_from_plain"], res["greedy"]


def test_kernel_matches_restatement(big, dev):
    """opus_debug_logits_process at V 96 / 128 256 / 152 064, B 1 and 64, histories up to 256 ids with repeats, penalties 0.8 /
    1.3 / 2.0, n 1 to 4, bad words of 1 to 8 ids: the processed logits bit for bit, untouched entries bit-identical."""
    res = lpc.kernel(big, dev)
    record("logits_proc.kernel", res)
    _check_kernel(res)


def test_micro_matches_reference_fixture(micro):
    """Each option of the fixture (penalties 1.3 and 0.8, n = 2, bad words, min_new_tokens, min_length) and a combined case: ids bit-exact up to each row's first step whose processed top-1
    margin is <= 0.05 in the reference's scores; scores within REL_L2 with the same -inf pattern; logits raw."""
    res = lpc.golden(micro)
    record("logits_proc.golden", res)
    assert set(res) == {"plain", "pen13", "pen08", "ngram2", "minnew", "bad", "minlen", "combo"}
    for tag, r in res.items():
        assert r["ids_ok"], (tag, r)
        assert r["inf_pattern_equal"], (tag, r)
        assert r["scores_rel_l2"] < REL_L2 and r["logits_rel_l2"] < REL_L2, (tag, r)


def test_llama8b_shape_greedy_and_sampling(big, dev):
    """Batch 64, 16 steps, every processor on: greedy ids are the arg-max of the restatement of the raw logits, sampled scores
    are the warpers after the restatement, token_logprobs stay raw (including chosen ids a penalty changed)."""
    res = lpc.big(big, dev, B=64, max_new=16)
    record("logits_proc.big", res)
    _check_big(res)


def test_graphs_and_default_path(big, dev):
    res = lpc.graphs(big, dev)
    record("logits_proc.graphs", res)
    assert res["plain_equal"] and res["plain_new_graphs"] == 0 and res["plain_replays"] > 0, res
    assert res["proc_graphs_second"] == 0, res                     # new values, same graph
    assert res["proc_changed_ids"], res
    assert res["timing_off_launches"] == 0 and res["timing_on_launches"] == 4, res


def test_early_stop_with_processors(micro):
    res = lpc.early_stop(micro, dict(np.load(os.path.join(GOLD, "generate_micro.npz"))))
    record("logits_proc.early_stop", res)
    for k, r in res.items():
        assert r["n"] < 12 and r["decode_steps"] <= r["n"] + 2, (k, r)


def test_bf16_build_logits_proc():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_logits_proc_check.py")], capture_output=True, text=True,
                       env=env, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_LOGITS_PROC ")][-1]
    o = json.loads(line[len("BF16_LOGITS_PROC "):])
    record("logits_proc.bf16", o)
    assert o["operand_dtype"] == 1, o
    _check_kernel(o["kernel"])
    for mode, r in o["big"].items():
        assert r["lp_abs"] <= SELF_ABS and r["argmax_mismatch"] == 0 and r["scores_mismatch"] == 0, (mode, r)
