"""generate(num_return_sequences=N) on the GPU: N answers per protein from one prefill.

The fanned-out prefill (opus_llama_prefill_fanout) runs the B prompts once and leaves B N decoder rows; everything it copies is
checked bit for bit - the first-step logits against the plain B-row prefill, the N replicas of a prompt against each other over
decode steps on a context dirtied by another batch - and every sampled id against the fp64 rule with the draw of its decoder row.
The only tolerances are those of comparisons between DIFFERENT launch shapes, taken from the project's existing rows:
  replica 0 vs a prefill of the prompts repeated N times (other prefill GEMM routes, same decode launches): the "a row of the batch
    vs that row alone" logits bound of tests/test_gpu_batch64.py at Llama-3-8B widths, the micro models' REL_L2 of
    tests/test_gpu_parity.py;
  token_logprobs vs score_continuations: DECODE_VS_PREFILL of tests/test_gpu_gen_scores.py;
  beam scores vs the reference's fixture: atol 2e-2 of tests/test_gpu_parity.py::test_generate_beam_golden;
  bf16: the logits row of DESIGN.md section 9 (tests/test_gpu_bf16.py).
Observed values are kept through gpu_helpers.record (those of the MI355X run are committed as profiles/nsamples_parity.jsonl).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import gen_scores_checks as gsc
import nsamples_checks as nsc
from gpu_helpers import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROW_VS_BATCH_LOGITS = 3e-3     # Llama-3-8B widths (tests/test_gpu_batch64.py)
MICRO_REL_L2 = 1.5e-2          # micro models (tests/test_gpu_parity.py REL_L2)
DECODE_VS_PREFILL = 1.5e-2     # tests/test_gpu_gen_scores.py
BEAM_SCORE_ATOL = 2e-2         # tests/test_gpu_parity.py::test_generate_beam_golden
BEAM_GAP = 0.04                # twice the score bound: hypotheses further apart than this keep their order
BF16_LOGITS = 2e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_MODELS = {}


def _micro(name, dev):
    if name not in _MODELS:
        _MODELS[name] = nsc.micro_model(name, dev)
    return _MODELS[name]


def _big(dev):
    if "llama8b" not in _MODELS:
        _MODELS["llama8b"] = gsc.make_model(gsc.llama8b_shape(64, 2, 8), dev)
    return _MODELS["llama8b"]


# ------------------------------------------------------------------------------------------------ (a) the reference's fixture
def _check_hypotheses(out, scores, want_ids, want_scores, B, N, pad):
    """out [B N, n] / scores [B N] against the fixture's [B, K, L] / [B, K]: by position where the fixture's score gaps to both
    neighbours exceed BEAM_GAP, as a set within a run of closer scores; returns how many were held by position."""
    n = out.shape[1]
    got = out.cpu().numpy().reshape(B, N, n)
    assert bool((want_ids[:, :N, n:] == pad).all())                  # cropped to the longest returned hypothesis
    np.testing.assert_allclose(scores.numpy().reshape(B, N), want_scores[:, :N], atol=BEAM_SCORE_ATOL)
    K = want_scores.shape[1]
    by_position = 0
    for b in range(B):
        k = 0
        while k < N:
            e = k
            while e + 1 < K and want_scores[b, e] - want_scores[b, e + 1] <= BEAM_GAP:
                e += 1                                               # hypotheses k .. e of the fixture are a near-tie run
            if e == k:
                assert np.array_equal(got[b, k], want_ids[b, k, :n]), (b, k, got[b], want_ids[b])
                by_position += 1
            else:
                pool = {tuple(want_ids[b, j, :n]) for j in range(k, e + 1)}
                mine = [tuple(got[b, j]) for j in range(k, min(e, N - 1) + 1)]
                assert len(set(mine)) == len(mine) and set(mine) <= pool, (b, k, e, got[b], want_ids[b])
                if e < N:
                    assert set(mine) == pool, (b, k, e, got[b], want_ids[b])
            k = e + 1
    return by_position


def test_beam_search_returns_all_hypotheses_of_the_fixture(dev, gold, gold_dir):
    """(a) generate(num_beams=3, num_return_sequences=3) on the inputs of generate_micro against the reference's own three
    hypotheses per row (tests/golden/generate_beam.npz, made with num_return_sequences=3), decoding to max_new_tokens and with the
    fixture's EOS id; num_return_sequences=2 gives the first two."""
    model = gsc.make_model(opa.micro(max_batch=12), dev)           # (seed 0: the weights the fixture was made with)
    g, base = gold("generate_beam"), gold("generate_micro")
    seqs = json.load(open(os.path.join(gold_dir, "generate_micro.seqs.json")))
    ids, mask = torch.from_numpy(base["ids"]), torch.from_numpy(base["mask"])
    pad, K, L, eos = int(base["pad"]), int(g["K"]), int(g["N"]), int(g["eos"])
    B = ids.shape[0]
    kw = dict(attention_mask=mask, pad_token_id=pad, do_sample=False, num_beams=K, max_new_tokens=L, return_dict_in_generate=True)
    held = {}
    for tag, extra, want_ids, want_sc in (("free", {}, g["free_ids"], g["free_scores"]),
                                          ("eos", dict(eos_token_id=[eos]), g["eos_ids"], g["eos_scores"])):
        o3 = model.generate(ids, seqs, num_return_sequences=K, **kw, **extra)
        assert o3.sequences.shape[0] == B * K and o3.sequences_scores.shape == (B * K,)
        held[tag] = _check_hypotheses(o3.sequences, o3.sequences_scores.cpu(), want_ids, want_sc, B, K, pad)
        o2 = model.generate(ids, seqs, num_return_sequences=2, **kw, **extra)
        n2 = o2.sequences.shape[1]
        first_two = o3.sequences.view(B, K, -1)[:, :2]
        assert o2.sequences.shape[0] == B * 2 and torch.equal(o2.sequences.view(B, 2, n2), first_two[:, :, :n2])
        assert bool((first_two[:, :, n2:] == pad).all())
        assert torch.equal(o2.sequences_scores.view(B, 2), o3.sequences_scores.view(B, K)[:, :2])
        _check_hypotheses(o2.sequences, o2.sequences_scores.cpu(), want_ids, want_sc, B, 2, pad)
        o1 = model.generate(ids, seqs, **kw, **extra)                # without the argument: the best one, as before
        n1 = o1.sequences.shape[1]
        assert torch.equal(o1.sequences, o3.sequences.view(B, K, -1)[:, 0, :n1])
    record("nsamples_beam_fixture", held)
    assert held == {"free": 7, "eos": 5}, held                       # (the fixture's gaps: 7 of 9 and 5 of 9 hypotheses by position)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, seqs, num_return_sequences=K + 1, **kw)


# ------------------------------------------------------------------------------------------------ (b), (c) exact copies
def _assert_replicas(o, bound):
    assert o["finite"] and o["first_exact"] and o["last_logits_exact"], o
    assert o["replicas_exact"] and o["prompts_differ"], o
    assert o["replica0_vs_repeated_rel_l2"] <= bound, o


@pytest.mark.parametrize("name", list(nsc.MICRO_CASES))
def test_fanout_prefill_logits_and_replicas_micro(dev, name):
    """(b) + (c) on the micro decoders (Llama, OPT, Qwen2): 4, 9, 63 and 8 decoder rows, ragged left-padded prompts."""
    model, B, N, lens = _micro(name, dev)
    o = nsc.prefill_and_replicas(model, dev, B, N, lens)
    record("nsamples_replicas", dict(case=name, **o))
    _assert_replicas(o, MICRO_REL_L2)
    assert o["T_dirty"] > o["T"], o                                   # the context was dirtied by longer prompts
    if name == "micro_7x9":
        assert o["pad_slots_max"] >= 33, o                            # a prompt padded by more than a key tile
    if name == "micro_2x2":
        assert o["T"] == 30 and o["last_slot"] == 32, o               # the decode steps cross cache slot 31 -> 32


@pytest.mark.parametrize("name", list(nsc.BIG_CASES))
def test_fanout_prefill_logits_and_replicas_llama8b(dev, name):
    """(b) + (c) at Llama-3-8B widths: 12 x 5 = 60 rows (B > N: an in-place row fan-out would be caught) and 1 x 64."""
    B, N, lens = nsc.BIG_CASES[name]
    o = nsc.prefill_and_replicas(_big(dev), dev, B, N, lens)
    record("nsamples_replicas", dict(case=name, **o))
    _assert_replicas(o, ROW_VS_BATCH_LOGITS)


# ------------------------------------------------------------------------------------------------ (d), (e) draws and scores
def _assert_sampled(o, B, N, open_mode):
    assert o["rows"] == B * N and o["logits_rows"] == B * N and o["lp_shape"][0] == B * N, o
    assert o["draws"] > 0 and o["mismatches"] == 0 and o["inadmissible"] == 0, o
    assert o["nondecisive"] < 1.0, o
    assert o["same_seed_equal"], o
    if open_mode:
        # temperature 1.0 over the whole vocabulary: another seed gives other ids, and the replicas of a prompt differ.  (In the
        # reference's mode the nucleus of top_p 0.7 at temperature 0.1 is often ONE token - then no draw can depend on the seed,
        # and four short rows may come out alike under every seed: recorded, not asserted.)
        assert o["other_seed_differs"], o
        if N > 1:
            assert not o["replicas_all_equal"], o


@pytest.mark.parametrize("mode", ["reference", "open"])
@pytest.mark.parametrize("name", list(nsc.MICRO_CASES))
def test_every_draw_matches_fp64_rule_micro(dev, name, mode):
    """(d) + (e), micro decoders, the reference's sampling mode (0.1 / 0.7 / 50) and (1.0 / 1.0 / 0)."""
    model, B, N, lens = _micro(name, dev)
    o = nsc.sampled(model, dev, B, N, lens, nsc.REFERENCE_MODE if mode == "reference" else nsc.OPEN_MODE)
    record("nsamples_sampled", dict(case=name, mode=mode, **o))
    _assert_sampled(o, B, N, mode == "open")
    assert o["teacher_forced_counted"] > 0 and o["teacher_forced_abs"] <= DECODE_VS_PREFILL, o


@pytest.mark.parametrize("mode", ["reference", "open"])
@pytest.mark.parametrize("name", list(nsc.BIG_CASES))
def test_every_draw_matches_fp64_rule_llama8b(dev, name, mode):
    """(d) + (e) at Llama-3-8B widths: the first token (drawn from the fanned-out prefill's logits) and one behind a decode step."""
    B, N, lens = nsc.BIG_CASES[name]
    o = nsc.sampled(_big(dev), dev, B, N, lens, nsc.REFERENCE_MODE if mode == "reference" else nsc.OPEN_MODE, max_new=2)
    record("nsamples_sampled", dict(case=name, mode=mode, **o))
    _assert_sampled(o, B, N, mode == "open")
    assert o["teacher_forced_counted"] > 0 and o["teacher_forced_abs"] <= DECODE_VS_PREFILL, o


# ------------------------------------------------------------------------------------------------ (f) per-row machinery
def test_eos_acts_per_decoder_row(dev):
    model, B, N, lens = _micro("micro_3x3", dev)
    o = nsc.eos_rows(model, dev, B, N, lens)
    record("nsamples_eos", o)
    assert o["rows"] == B * N and 0 < o["finished_rows"] < o["rows"], o
    assert o["rows_ok"] and o["n"] == o["longest"], o


def test_logits_processors_act_per_decoder_row(dev):
    model, B, N, lens = _micro("micro_3x3", dev)
    o = nsc.processors(model, dev, B, N, lens)
    record("nsamples_processors", o)
    assert o["rows"] == B * N and o["ngram_bans"] > 0, o
    assert o["scores_mismatch"] == o["mismatch_near_threshold"] and o["drawn_not_finite"] == 0, o


def test_per_row_tries_follow_their_prompt(dev):
    model, B, N, lens = _micro("micro_3x3", dev)
    o = nsc.per_row_tries(model, dev, B, N, lens)
    record("nsamples_tries", o)
    assert o["rows"] == B * N and o["disjoint_tries"] and o["accepted"], o


def test_errors_and_capacity(dev):
    from opus_pllm_amd import _cabi
    model, B, N, lens = _micro("micro_3x3", dev)
    ids, mask, seqs = nsc.prompts(model.cfg, lens)
    kw = dict(attention_mask=mask, pad_token_id=nsc.PAD, max_new_tokens=3)
    with pytest.raises(ValueError, match="Greedy methods without beam search"):
        model.generate(ids, seqs, num_return_sequences=2, **kw)
    with pytest.raises(ValueError):
        model.generate(ids, seqs, num_return_sequences=0, do_sample=True, **kw)
    with pytest.raises(_cabi.OpusError):
        model.generate(ids, seqs, num_return_sequences=4, do_sample=True, **kw)         # 12 rows > max_batch = 9
    emb, m = nsc.spliced(model, ids, mask, seqs)
    with pytest.raises(_cabi.OpusError):
        model.prefill_logits(emb, m, num_return_sequences=4)                           # the C entry refuses it too
    out = model.generate(ids, seqs, num_return_sequences=3, do_sample=True, seed=1, **kw)
    assert out.shape == (9, 3)                                                           # (and the context is usable afterwards)


# ------------------------------------------------------------------------------------------------ (g) N = 1 is today's call
def test_one_return_sequence_is_the_plain_call(dev):
    model, B, N, lens = _micro("micro_3x3", dev)
    o = nsc.n1_is_plain(model, dev, B, lens)
    record("nsamples_n1", o)
    for tag in ("greedy", "sample"):
        r = o[tag]
        assert r["ids_equal"] and r["new_graphs"] == 0, o
        assert r["replays_one"] == r["replays_plain"] and r["steps_one"] == r["steps_plain"], o
        assert r["launches_one"] == r["launches_plain"] and r["launches_plain"] > 0, o
    assert o["after_nsample"]["rows"] == B * o["after_nsample"]["N"] and o["after_nsample"]["plain_equal"], o


# ------------------------------------------------------------------------------------------------ the driver
def test_eval_loop_num_return_sequences():
    """eval_ddp.annotate(num_return_sequences=3) (--num_return_sequences): batch_size // 3 prompts per call, 3 rows per item in item
    order; a seed reproduces them; the log-probabilities and the last logits have 3 rows per item too."""
    import importlib.util
    from opus_pllm_amd import builder, synth
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=6,
                                                  max_enc_tokens=258, max_prompt=64, max_new_tokens=8)
    items = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(20 + 11 * (i % 9), i), output="x")
             for i in range(5)]
    kw = dict(temperature=1.0, top_p=1.0, inflight=1, num_return_sequences=3)
    torch.manual_seed(3)
    lps, logits = [], []
    a = ddp.annotate(model, tok, items, "", 6, 8, logprobs_out=lps, logits_out=logits, **kw)
    torch.manual_seed(3)
    b = ddp.annotate(model, tok, items, "", 6, 8, **kw)
    assert a.shape == (5 * 3, 8) and torch.equal(a, b)
    assert [x[0].shape[0] for x in lps] == [6, 6, 3] and [x.shape[0] for x in logits] == [6, 6, 3]     # 2, 2 and 1 prompts per call
    rows = a.view(5, 3, 8)
    assert any(not torch.equal(rows[i, 0], rows[i, j]) for i in range(5) for j in (1, 2))               # the answers of an item differ
    texts = tok.batch_decode(a, skip_special_tokens=True)
    res = ddp.build_result(items, texts, 3)
    assert len(res) == 5 and all(len(r["generated_all"]) == 3 and r["generated"] == r["generated_all"][0] for r in res)


# ------------------------------------------------------------------------------------------------ bf16
def test_bf16_build_nsamples():
    """(b), (c) and (d) on the bf16-operand build, in a fresh child process (the library choice is per process): the exact checks
    stay exact, replica 0 vs the repeated prompts within the bf16 logits bound."""
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_nsamples_check.py")], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_NSAMPLES ")][-1]
    o = json.loads(line[len("BF16_NSAMPLES "):])
    record("nsamples_bf16", o)
    assert o["operand_dtype"] == 1, o
    for case, (B, N) in (("micro_3x3", (3, 3)), ("llama8b_12x5", (12, 5))):
        _assert_replicas(o[case]["replicas"], BF16_LOGITS)
        _assert_sampled(o[case]["reference_mode"], B, N, False)
        _assert_sampled(o[case]["open_mode"], B, N, True)
