"""GPU tests of generate(return_dict_in_generate=True, output_scores / output_logits / output_token_logprobs): the reference's own
scores (tests/golden/generate_scores_micro.npz, tools/gen_golden_scores.py), the fused arg-max / log-sum-exp kernel, self-
consistency at the Llama-3-8B vocabulary and batch 64, unchanged ids and graphs, the sampling filter, ragged finishes,
forward(labels=...) and beams.  Nothing here reads the reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import gen_scores_checks as gsc
from gpu_helpers import record, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REL_L2 = 1.5e-2            # logits vs the fp32 reference (tests/test_gpu_forward.py)
TRANSITION_ABS = 2e-2      # normalised transition scores vs the reference's
LSE_REL = 1e-5             # kernel: |lse - fp64| <= LSE_REL * max(1, |lse|)
SELF_ABS = 1e-5            # token_logprobs vs fp64 log_softmax of the returned logits
DECODE_VS_PREFILL = 1.5e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _gold(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


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
    cfg = gsc.llama8b_shape(B=64, layers=2, max_new=8)
    return gsc.make_model(cfg, dev)


def _micro_inputs():
    g = _gold("generate_micro")
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    return g, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), seqs


def test_scores_match_reference_fixture(micro):
    """Greedy with output_scores + output_logits against the reference's generate(return_dict_in_generate=True, ...): the ids,
    the scores and logits of every step, and compute_transition_scores(normalize_logits=True); to max_new_tokens and with an EOS
    that finishes rows at different steps."""
    gs = _gold("generate_scores_micro")
    _, ids, mask, seqs = _micro_inputs()
    N, pad = int(gs["N"]), int(gs["pad"])
    seen = {}
    for tag, eos in (("free", None), ("eos", [int(gs["eos_id"])])):
        out = micro.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, use_cache=True,
                             eos_token_id=eos, return_dict_in_generate=True, output_scores=True, output_logits=True)
        assert type(out).__name__ == "GenerateDecoderOnlyOutput"
        assert np.array_equal(out.sequences.cpu().numpy(), gs[tag + ".sequences"]), tag
        assert len(out.scores) == len(out.logits) == out.sequences.shape[1] == gs[tag + ".scores"].shape[0]
        sc, lg = torch.stack(out.scores).cpu(), torch.stack(out.logits).cpu()
        e_sc, e_lg = rel_l2(sc, torch.from_numpy(gs[tag + ".scores"])), rel_l2(lg, torch.from_numpy(gs[tag + ".logits"]))
        tr = micro.compute_transition_scores(out.sequences, out.logits, normalize_logits=True).cpu()
        e_tr = float((tr - torch.from_numpy(gs[tag + ".transition"])).abs().max())
        seen[tag] = dict(scores_rel_l2=e_sc, logits_rel_l2=e_lg, transition_abs=e_tr)
        assert e_sc < REL_L2 and e_lg < REL_L2 and e_tr < TRANSITION_ABS, (tag, seen[tag])
    record("gen_scores.fixture", seen)


def test_argmax_lse_kernel(micro, dev):
    res = gsc.argmax_lse_kernel(micro, dev)
    record("gen_scores.kernel", res)
    for name, r in res.items():
        assert r["idx_bitwise"] and r["lse_rel"] < LSE_REL, (name, r)


def test_self_consistency_llama8b_batch64(big, dev):
    res = gsc.self_consistency(big, dev, B=64, max_new=8)
    record("gen_scores.self_consistency", res)
    _check_self(res)


def _check_self(res):
    for mode, r in res.items():
        assert r["ids_equal_all_flags"], (mode, r)
        assert r["plain_replays"] > 0 and r["plain_new_graphs"] == 0, (mode, r)
        assert r["lp_abs"] < SELF_ABS and r["transition_abs"] < SELF_ABS, (mode, r)
        assert r["zero_after_end"] and r["logprob_sum_abs"] < 1e-3, (mode, r)
        assert r["len_scores"] == r["len_logits"] == r["n"], (mode, r)
        assert r["scores_is_logits"] == (mode == "greedy"), (mode, r)
        if mode != "greedy":
            assert r["filter_mismatch"] == r["filter_mismatch_near_threshold"], (mode, r)
            assert r["drawn_finite_steps"] == r["n"], (mode, r)
            assert r.get("scores_value_rel", 0.0) < 1e-6, (mode, r)


def test_ragged_finish(micro):
    res = gsc.ragged(micro, None, _gold("generate_micro"))
    record("gen_scores.ragged", res)
    for tag, r in res.items():
        assert r["ids_equal"] and r["ragged"], (tag, r)
        assert r["len_scores"] == r["n"] and max(r["n_tokens"]) == r["n"], (tag, r)
        assert r["zero_after_end"] and r["logprob_ok"], (tag, r)
    assert res["eos"]["n"] < res["eos"]["N"]                   # every row finished: the batch stopped early


def test_token_logprobs_match_forward_labels(micro):
    """The generated ids fed back as labels behind the same prompts: forward()'s token_logprobs at those positions equal
    generate()'s to the decode-vs-prefill bound."""
    g, ids, mask, seqs = _micro_inputs()
    pad, N = int(g["pad"]), 10
    eos = [int(g["eos"])]
    o = micro.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, eos_token_id=eos,
                       return_dict_in_generate=True, output_token_logprobs=True)
    gen, cnt, lp = o.sequences.cpu(), o.n_tokens.cpu(), o.token_logprobs.cpu()
    rows, labs = [], []
    for b in range(ids.shape[0]):
        prompt = ids[b][mask[b]].tolist()
        ans = gen[b, : int(cnt[b])].tolist()
        rows.append(prompt + ans)
        labs.append([-100] * len(prompt) + ans)
    W = max(len(r) for r in rows)
    fids = torch.full((len(rows), W), pad, dtype=torch.long)
    flab = torch.full((len(rows), W), -100, dtype=torch.long)
    fmask = torch.zeros((len(rows), W), dtype=torch.bool)
    for b, (r, l) in enumerate(zip(rows, labs)):
        fids[b, : len(r)], flab[b, : len(l)], fmask[b, : len(r)] = torch.tensor(r), torch.tensor(l), True
    out = micro.forward(fids, attention_mask=fmask, labels=flab, seq=seqs)
    _, _, _, _, _, lab_out = micro.prepare_inputs_labels_for_multimodal(fids, None, fmask, None, flab, seqs)
    worst = 0.0
    for b in range(len(rows)):
        f = out.token_logprobs[b].cpu()[lab_out[b].cpu() != -100]
        n = int(cnt[b])
        assert f.numel() == n, (b, f.numel(), n)
        worst = max(worst, float((f - lp[b, :n]).abs().max()))
    record("gen_scores.vs_forward", worst)
    assert worst < DECODE_VS_PREFILL, worst


def test_beam_output(dev):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    from opus_pllm_amd import synth
    cfg = opa.micro(max_batch=12)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, 0), dev), dev)
    g, base = _gold("generate_beam"), _gold("generate_micro")
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    ids, mask = torch.from_numpy(base["ids"]), torch.from_numpy(base["mask"])
    kw = dict(attention_mask=mask, pad_token_id=int(base["pad"]), do_sample=False, num_beams=int(g["K"]),
              max_new_tokens=int(g["N"]), use_cache=True)
    out = model.generate(ids, seqs, return_dict_in_generate=True, **kw)
    assert type(out).__name__ == "GenerateBeamDecoderOnlyOutput" and out.keys() == ["sequences", "sequences_scores"]
    assert np.array_equal(out.sequences.cpu().numpy(), g["free_ids"][:, 0])
    assert torch.equal(out.sequences_scores.cpu(), model.last_beam_scores)
    np.testing.assert_allclose(out.sequences_scores.cpu().numpy(), g["free_scores"][:, 0], atol=2e-2)
    with pytest.raises(NotImplementedError):
        model.generate(ids, seqs, return_dict_in_generate=True, output_scores=True, **kw)


def test_flags_ignored_without_return_dict(micro):
    _, ids, mask, seqs = _micro_inputs()
    kw = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=6)
    a = micro.generate(ids, seqs, **kw)
    i0 = micro.stat("graph_instantiations")
    b = micro.generate(ids, seqs, output_scores=True, output_logits=True, output_token_logprobs=True, **kw)
    assert isinstance(b, torch.Tensor) and torch.equal(a, b) and micro.stat("graph_instantiations") == i0


def test_eval_loop_save_logprobs():
    """eval_ddp.annotate(logprobs_out=...) (--save_logprobs): the same ids as without it, greedy and sampling, and per item the
    counted log-probabilities (0 behind them)."""
    import importlib.util
    from opus_pllm_amd import builder, synth
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=258, max_prompt=64, max_new_tokens=8)
    items = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(20 + 11 * (i % 9), i), output="x")
             for i in range(7)]
    for temp in (0.0, 0.9):
        torch.manual_seed(3)
        plain = ddp.annotate(model, tok, items, "", 4, 8, temperature=temp, top_p=0.95)
        torch.manual_seed(3)
        lps = []
        with_lp = ddp.annotate(model, tok, items, "", 4, 8, temperature=temp, top_p=0.95, logprobs_out=lps)
        assert torch.equal(plain, with_lp), temp
        lp = torch.cat([x[0] for x in lps]).cpu()
        n = torch.cat([x[1] for x in lps]).cpu()
        assert lp.shape == (7, 8) and n.shape == (7,) and int(n.min()) >= 1
        pos = torch.arange(8)[None, :]
        assert bool((lp[pos >= n[:, None]] == 0).all()) and bool((lp[pos < n[:, None]] <= 0).all())


def test_bf16_build_gen_scores():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_gen_scores_check.py")], capture_output=True, text=True,
                       env=env, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_GEN_SCORES ")][-1]
    o = json.loads(line[len("BF16_GEN_SCORES "):])
    record("gen_scores.bf16", o)
    assert o["operand_dtype"] == 1, o
    for name, r in o["kernel"].items():
        assert r["idx_bitwise"] and r["lse_rel"] < LSE_REL, (name, r)
    _check_self(o["self"])
