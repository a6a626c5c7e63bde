"""GPU tests of generate(guidance_scale=...), classifier-free guidance on paired rows: the combine kernel against fp64
(opus_debug_guidance), the micro model against the fp32 oracle through the paired-row restatement (tests/guidance_ref.py, which
tests/test_guidance_host.py holds to the installed transformers), device against device (off switch, graphs, the doubled batch,
teacher-forced scores at the micro shape and at Llama-3-8B widths), the options on top, and the bf16 build.  Nothing here reads
the reference."""
import json
import os
import subprocess
import sys

import pytest
import torch

import guidance_checks as gc
import gen_scores_checks as gsc
import logits_proc_ref as lpr
from gpu_helpers import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO_REL = 1.5e-2         # the micro fixtures' generic rel-L2 bound of logits against fp32 (tests/test_gpu_constrained.py)
BIG_REL = 2e-3             # "decode equals prefill of the longer prompt" at Llama-3-8B widths
SELF_ABS = 1e-5            # token_logprobs vs fp64 log_softmax of the returned raw logits (tests/test_gpu_logits_proc.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def micro(dev):
    return gc.make_micro(dev)


@pytest.fixture(scope="module")
def big(dev):
    return gsc.make_model(gsc.llama8b_shape(B=64, layers=2, max_new=8), dev)


def _parity(name, value):
    """Observed maxima, kept through gpu_helpers.record (those of the MI355X run are committed as profiles/guidance_parity.jsonl)."""
    record("guidance." + name, value)


def check_kernel(res):
    for name, r in res.items():
        print(f"guidance kernel {name}: err={r['err']:.3e} err32={r['err32']:.3e} bound={r['bound']:.3e}")
        assert r["finite"], (name, r)
        assert r["equal_pair_exact"], (name, r)
        assert r["partners_unchanged"] and r["sentinels_unchanged"], (name, r)
        assert r["err"] <= r["bound"], (name, r)


@pytest.mark.parametrize("V", [1, 33, 96, 50001, 128256, 152064])
@pytest.mark.parametrize("P", [1, 3, 32])
def test_kernel_matches_fp64(micro, dev, P, V):
    """opus_debug_guidance (a 12-row context: P = 32 runs in chunks) for g in 0, 0.5, 1.5, 3, 7.5 on Gaussian logits x 4 with a
    common offset of 1e4, a peaked row and a bit-equal pair: |got - ref64| <= max(8 x the torch-fp32 form's own error, 1e-5), no
    -inf / NaN, the bit-equal pair exactly the device's own log-softmax, partner rows and sentinels bit-unchanged."""
    res = gc.kernel(micro[0], dev, shapes=[(P, V)])
    assert len(res) == len(gc.SCALES)
    _parity(f"kernel.P{P}_V{V}", {"err": max(r["err"] for r in res.values()), "err32": max(r["err32"] for r in res.values()),
                                  "worst_ratio_to_bound": max(r["err"] / r["bound"] for r in res.values())})
    check_kernel(res)


def test_micro_matches_fp32_oracle(micro):
    """Greedy, g = 1.5 and 3, proteins in the prompts, the protein-free twin and an explicit negative prompt, 8 new tokens, against
    the restatement over oracle/ logits.  The weights seed was chosen on the CPU (guidance_checks.choose_micro_seed): no seed keeps
    every step decisive, so the best one's decisive count is asserted exactly (83 of 96 >= 0.75).  ids equal on every decisive
    step; guided scores within MICRO_REL x 2 (2 g - 1) rel-L2 wherever the device still follows the oracle's ids."""
    model, canon = micro
    res = gc.micro_vs_oracle(model, canon)
    _parity("micro_vs_oracle", res)
    assert set(res) == {"g1.5_twin", "g1.5_explicit", "g3.0_twin", "g3.0_explicit"}
    n_dec = sum(round(r["decisive_fraction"] * 24) for r in res.values())
    assert (n_dec, 24 * len(res)) == gc.MICRO_DECISIVE and n_dec / (24 * len(res)) >= 0.75, res
    for tag, r in res.items():
        g = float(tag[1:].split("_")[0])
        print(f"guidance micro {tag}: {r}")
        assert r["shape"] == [3, gc.MICRO_NEW], (tag, r)
        assert r["ids_equal_on_decisive"], (tag, r)
        assert r["scores_compared"] >= 3 and r["scores_rel_l2"] <= gc.scores_bound(g, MICRO_REL), (tag, r)


def test_off_switch_graphs_and_doubled_batch(micro):
    """guidance_scale None / 1: ids bit-identical to the plain call, no graph instantiated; another scale: none either; text-only
    prompts with the negative prompt equal to the prompt: for every g the plain greedy ids of the doubled batch."""
    res = gc.off_switch_and_graphs(micro[0], B=4, max_new=8)
    _parity("off_switch", res)
    assert res["off_equal"] and res["off_new_graphs"] == 0 and res["plain_after_new_graphs"] == 0, res
    assert res["guided_graphs_first"] <= 1 and res["guided_graphs_other_scale"] == 0, res
    assert res["guided_repeatable"] and res["guided_differs_from_plain"] and res["scales_differ"], res
    assert res["doubled_halves_equal"] and all(res["equal_prompt_is_doubled_plain"].values()), res
    assert res["shape"] == [4, 8], res


def check_teacher_forced(tag, r, g, generic):
    bound = gc.scores_bound(g, generic)
    print(f"guidance teacher-forced {tag}: scores_rel_l2={r['scores_rel_l2']:.3e} logits_rel_l2={r['logits_rel_l2']:.3e} "
          f"bound={bound:.3e} mismatch_gaps={r['mismatch_gaps']} decided={r['decided']} lp_abs={r['lp_abs']:.3e}")
    assert r["inf_pattern_equal"], (tag, r)
    assert r["scores_rel_l2"] <= bound, (tag, r["scores_rel_l2"], bound)
    assert r["logits_rel_l2"] <= generic, (tag, r["logits_rel_l2"])          # `logits` stay raw and conditional
    assert all(gap <= bound for gap in r["mismatch_gaps"]), (tag, r["mismatch_gaps"], bound)   # the id is the arg-max where decided
    assert r["lp_abs"] <= SELF_ABS and r["zero_after_end"], (tag, r)          # token_logprobs: raw, conditional


@pytest.mark.parametrize("g", [1.5, 3.0])
def test_teacher_forced_micro(micro, g):
    """Every step's guided `scores` against the combine of the two prefill_logits of the prompts extended by the ids so far."""
    model, _ = micro
    ids, mask, seqs, neg, nmask = gc.micro_inputs(model.cfg)
    for tag, kw in (("twin", {}), ("explicit", dict(neg=neg, nmask=nmask))):
        r = gc.teacher_forced(model, ids, mask, seqs, g, gc.MICRO_NEW, **kw)
        _parity(f"teacher_forced.micro.g{g}.{tag}", {k: r[k] for k in ("scores_rel_l2", "logits_rel_l2", "mismatch_gaps", "decided", "lp_abs")})
        assert r["n"] == gc.MICRO_NEW and r["decided"] == 3 * gc.MICRO_NEW
        check_teacher_forced(f"micro g={g} {tag}", r, g, MICRO_REL)


@pytest.mark.parametrize("g", [1.5, 3.0])
def test_teacher_forced_llama8b_widths(big, g):
    """Llama-3-8B widths x 2 layers, P = 32 (64 decoder rows), 4 steps, proteins in the prompts, the protein-free twin."""
    ids, mask, seqs = gsc.batch(big.cfg, 32)
    r = gc.teacher_forced(big, ids, mask, seqs, g, 4)
    _parity(f"teacher_forced.llama8b.g{g}", {k: r[k] for k in ("scores_rel_l2", "logits_rel_l2", "mismatch_gaps", "decided", "lp_abs")})
    assert r["n"] == 4 and r["decided"] == 32 * 4
    check_teacher_forced(f"llama8b g={g}", r, g, BIG_REL)


def test_processors_on_top(micro):
    """repetition_penalty + no_repeat_ngram_size behind the guidance: the restatement over device logits, -inf pattern included."""
    model, _ = micro
    ids, mask, seqs, _, _ = gc.micro_inputs(model.cfg)
    # (n-gram size 1: no id twice - the unprocessed run repeats one, so the answer has to change)
    proc = lambda s, hist: lpr.process(s, hist, penalty=1.3, ngram=1)          # noqa: E731
    r = gc.teacher_forced(model, ids, mask, seqs, 2.0, gc.MICRO_NEW, process=proc, repetition_penalty=1.3, no_repeat_ngram_size=1)
    _parity("teacher_forced.micro.processors", {k: r[k] for k in ("scores_rel_l2", "mismatch_gaps", "lp_abs")})
    check_teacher_forced("micro processors", r, 2.0, MICRO_REL)
    plain = model.generate(ids, seqs, attention_mask=mask, pad_token_id=gc.PAD, max_new_tokens=gc.MICRO_NEW, guidance_scale=2.0)
    assert all(len(set(row)) == len(row) for row in r["ids"]), r["ids"]
    assert r["ids"] != plain.cpu().tolist()                                   # the processors changed the answer


def test_options_on_top(micro):
    res = gc.options(micro[0])
    _parity("options", {k: v for k, v in res.items() if k != "eos"})
    assert res["sampling"] == {"reproduces": True, "other_seed_differs": True, "shape": [3, gc.MICRO_NEW]}, res["sampling"]
    assert res["trie"]["members_only"] and res["trie"]["inf_outside_allowed"], res["trie"]
    e = res["eos"]
    check_teacher_forced("micro eos", e, 2.0, MICRO_REL)                      # scores of finished rows too: partners were fed pads
    # what the free run's ids imply: a row ends with its first EOS id, pads follow, the call is cut where the last row ended
    want_cnt = [next((t + 1 for t, x in enumerate(row) if x in e["eos"]), len(row)) for row in e["free"]]
    assert len(set(want_cnt)) > 1 and min(want_cnt) < gc.MICRO_NEW, want_cnt
    assert e["n"] == max(want_cnt) and e["n_tokens"] == want_cnt, (e["n"], e["n_tokens"], want_cnt)
    for row, free, c in zip(e["ids"], e["free"], want_cnt):
        assert row[:c] == free[:c] and row[c:] == [gc.PAD] * (e["n"] - c), (row, free, c)
    assert res["stop"]["row0_stops"] and res["stop"]["others_unchanged"], res["stop"]
    t = res["timing"]
    assert t["off_launches"] == 0 and t["on_launches"] == 4 * t["steps"], t   # lse partial + final, combine, partner token
    assert res["raises"] == {"raised": [True, True, True], "works_afterwards": True}, res["raises"]


def test_bf16_build_guidance():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_guidance_check.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_GUIDANCE ")][-1]
    o = json.loads(line[len("BF16_GUIDANCE "):])
    _parity("bf16", {"kernel_worst_ratio": max(v["err"] / v["bound"] for v in o["kernel"].values()),
                     "teacher_forced": {k: {q: v[q] for q in ("scores_rel_l2", "logits_rel_l2", "mismatch_gaps")} for k, v in o["teacher_forced"].items()}})
    assert o["operand_dtype"] == 1, o
    assert len(o["kernel"]) == 18 * len(gc.SCALES)
    check_kernel(o["kernel"])
    assert set(o["teacher_forced"]) == {"g1.5", "g3.0"}
    for tag, r_ in o["teacher_forced"].items():
        check_teacher_forced("bf16 micro " + tag, r_, float(tag[1:]), 2e-2)   # the bf16 row's generic bound in place of 1.5e-2
