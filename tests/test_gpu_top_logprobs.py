"""GPU tests of top log-probs: the two-stage selection kernel through opus_debug_top_logprobs against the fp64 restatement
(tests/top_logprobs_ref.py), generate(top_logprobs=k) against the top-k recomputed from the raw logits the same call returns -
greedy, sampling, processors, a TokenTrie, guidance, num_return_sequences, behind a prefix, the OPT and Qwen2 families, the
Llama-3-8B width - unchanged ids and graphs, ragged finishes, and forward(labels, top_logprobs=k).  The bounds are those of
tests/test_gpu_gen_scores.py; ids are compared exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import gen_scores_checks as gsc
import top_logprobs_checks as tlc
import top_logprobs_ref as tref
from gpu_helpers import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LSE_REL = 1e-5             # kernel: |lp - fp64| <= LSE_REL * max(1, |lse|)          (tests/test_gpu_gen_scores.py)
SELF_ABS = 1e-5            # against fp64 on the returned logits                      (tests/test_gpu_gen_scores.py)
DECODE_VS_PREFILL = 1.5e-2
SAMPLING = dict(temperature=1.0, top_p=0.9, top_k=50)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _model(cfg, dev):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    from opus_pllm_amd import synth
    return OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, 0), dev), dev)


@pytest.fixture(scope="module")
def micro(dev):
    return _model(opa.micro(max_batch=12), dev)


@pytest.fixture(scope="module")
def big(dev):
    return gsc.make_model(tlc.llama8b_shape(B=64, layers=2, max_new=8), dev)


def _micro_inputs():
    g = dict(np.load(os.path.join(GOLD, "generate_micro.npz")))
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    return g, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), seqs


def _check_kernel(res):
    for name, r in res.items():
        assert r["id_mismatches"] == 0 and r["lp_rel"] <= LSE_REL, (name, r)
        assert r.get("ids_are_first", True) and r.get("lp_abs", 0.0) <= LSE_REL * max(1.0, np.log(128256)), (name, r)
        assert r.get("inf_tail", True), (name, r)


@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "h16"])
@pytest.mark.parametrize("V", [96, 1043, 32000, 128256])
def test_kernel_against_fp64(micro, dev, V, f32):
    """(the context holds 12 rows: R = 64 also walks the entry point's row groups)"""
    res = tlc.kernel_cases(micro, dev, V, f32)
    record(f"top_logprobs.kernel.V{V}.{'fp32' if f32 else 'h16'}", res)
    _check_kernel(res)


def test_kernel_argument_errors(micro, dev):
    from opus_pllm_amd import _cabi
    lib = _cabi.lib()
    x = torch.zeros(2 * 96, dtype=torch.float32, device=dev)
    ids = torch.zeros(2 * 20, dtype=torch.int32, device=dev)
    lp = torch.zeros(2 * 20, dtype=torch.float32, device=dev)
    call = lambda dtype, ld, R, V, k: lib.opus_debug_top_logprobs(micro._ctx, x.data_ptr(), dtype, ld, R, V, k, None, ids.data_ptr(),   # noqa: E731
                                                                  lp.data_ptr(), None)
    assert call(_cabi.OPUS_F32, 96, 2, 96, 0) == -1 and call(_cabi.OPUS_F32, 96, 2, 96, 21) == -1 and call(_cabi.OPUS_F32, 8, 2, 8, 9) == -1
    assert call(_cabi.OPUS_I32, 96, 2, 96, 5) == -1 and call(_cabi.OPUS_F32, 95, 2, 96, 5) != 0
    assert lib.opus_set_gen_top_logprobs(micro._ctx, 21, ids.data_ptr(), lp.data_ptr()) == -1
    assert lib.opus_set_gen_top_logprobs(micro._ctx, 5, None, lp.data_ptr()) == -1
    assert lib.opus_set_gen_top_logprobs(micro._ctx, 0, None, None) == 0


def _check_self(name, r, plain_path, greedy_plain=False):
    assert r["id_mismatches"] == 0 and r["lp_abs"] < SELF_ABS and r["tail_ok"], (name, r)
    assert r["chosen_seen"] > 0 and r["chosen_abs"] < SELF_ABS, (name, r)
    if plain_path:
        assert r["chosen_bitwise"], (name, r)
    if greedy_plain:
        assert r["top1_is_id"], (name, r)


def test_micro_self_consistency(micro):
    _, ids, mask, seqs = _micro_inputs()
    res = {}
    for name, k, samp, kw, plain in (("greedy", 5, None, {}, True), ("greedy_k20", 20, None, {}, True), ("sampled", 5, SAMPLING, {}, True),
                                     ("processors", 5, None, dict(repetition_penalty=1.3, no_repeat_ngram_size=2), False),
                                     ("processors_sampled", 4, SAMPLING, dict(repetition_penalty=1.3, no_repeat_ngram_size=2), False),
                                     ("guided", 5, None, dict(guidance_scale=1.5), False),
                                     ("guided_sampled", 3, SAMPLING, dict(guidance_scale=1.5), False),
                                     ("nret3", 5, SAMPLING, dict(num_return_sequences=3), True)):
        o = tlc.gen(micro, ids, mask, seqs, 8, k=k, sampling=samp, **kw)
        assert o.top_ids.shape[0] == ids.shape[0] * kw.get("num_return_sequences", 1)
        res[name] = tlc.consistency(o, k, plain)
        _check_self(name, res[name], plain, greedy_plain=name.startswith("greedy"))
    record("top_logprobs.micro", res)


def test_micro_token_trie(micro):
    from opus_pllm_amd.constraint import TokenTrie
    _, ids, mask, seqs = _micro_inputs()
    trie = TokenTrie([[5, 9, 11], [5, 9, 40, 41], [60, 61], [7]], end_token_id=3)
    for samp in (None, SAMPLING):
        o = tlc.gen(micro, ids, mask, seqs, 8, k=5, sampling=samp, prefix_allowed_tokens_fn=trie, eos_token_id=3)
        r = tlc.consistency(o, 5, False)
        # the alternatives are those of the raw row: the chosen id need not be among them under a constraint
        assert r["id_mismatches"] == 0 and r["lp_abs"] < SELF_ABS and r["tail_ok"] and r["chosen_abs"] < SELF_ABS, r


def test_behind_prefix(micro):
    import prefix_generate_checks as pgc
    cfg = micro.cfg
    src = [0, 1, 1, 0]
    pre, suf, _ = pgc.text_batch(cfg, [9, 14], [4, 6, 3, 5], src, 3)
    pids, pmask = pgc.left_pad(pre)
    prefix = micro.cache_prefix(pids, attention_mask=pmask, detach=True)
    sids, smask = pgc.left_pad(suf)
    for samp in (None, SAMPLING):
        kw = dict(do_sample=True, seed=11, **samp) if samp else {}
        o = micro.generate(sids, attention_mask=smask, prefix=prefix, prefix_rows=torch.tensor(src), pad_token_id=pgc.PAD, max_new_tokens=6,
                           return_dict_in_generate=True, output_logits=True, output_token_logprobs=True, top_logprobs=5, **kw)
        _check_self("behind", tlc.consistency(o, 5, True), True, greedy_plain=samp is None)
    o = micro.generate(sids, attention_mask=smask, prefix=prefix, prefix_rows=torch.tensor(src), pad_token_id=pgc.PAD, max_new_tokens=6,
                       return_dict_in_generate=True, output_logits=True, output_token_logprobs=True, top_logprobs=5, return_prefix=True)
    _check_self("return_prefix", tlc.consistency(o, 5, True), True, greedy_plain=True)
    assert o.prefix is not None


@pytest.mark.parametrize("family", ["micro_opt", "micro_qwen"])
def test_families(dev, family):
    cfg = opa.PRESETS[family](max_batch=8)
    model = gsc.make_model(cfg, dev)
    ids, mask, seqs = gsc.batch(cfg, 5)
    for samp in (None, SAMPLING):
        r = tlc.consistency(tlc.gen(model, ids, mask, seqs, 6, k=5, sampling=samp), 5, True)
        _check_self(family, r, True, greedy_plain=samp is None)


def test_c1_tiny(dev):
    cfg = opa.c1_tiny()
    model = gsc.make_model(cfg, dev)
    ids, mask, seqs = gsc.batch(cfg, 6)
    res = {}
    for name, k, samp, kw, plain in (("greedy", 20, None, {}, True), ("sampled", 5, SAMPLING, {}, True),
                                     ("processors", 5, SAMPLING, dict(repetition_penalty=1.2, no_repeat_ngram_size=3), False)):
        res[name] = tlc.consistency(tlc.gen(model, ids, mask, seqs, 8, k=k, sampling=samp, **kw), k, plain)
        _check_self(name, res[name], plain, greedy_plain=name == "greedy")
    record("top_logprobs.c1_tiny", res)


def test_ids_and_graphs(micro):
    _, ids, mask, seqs = _micro_inputs()
    for samp in (None, SAMPLING):
        r = tlc.graphs(micro, ids, mask, seqs, 8, samp)
        assert r["ids_equal"] and r["k7_new_graphs"] == 0 and r["plain_new_graphs"] == 0, r
        assert r["k3_prefix_of_k7"] and r["ignored_is_tensor"] and r["only_top_fields"], r


def test_ragged_finish(micro):
    """Several EOS ids, then a stop sequence: rows end at different steps; -1 / 0 behind each row's end, the step that ends a row
    still counts, the ids are those of the plain call."""
    g, ids, mask, seqs = _micro_inputs()
    free = torch.from_numpy(g["free_ids"])
    N, pad = free.shape[1], int(g["pad"])
    cases = {"eos": dict(eos_token_id=[int(free[0, 3]), int(free[1, 4]), int(free[2, 5])]),
             "stop": dict(stop_sequence=[int(free[0, 1]), int(free[0, 2])], eos_token_id=[int(free[2, 6])])}
    for tag, kw in cases.items():
        base = dict(attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, **kw)
        o = micro.generate(ids, seqs, return_dict_in_generate=True, output_logits=True, output_token_logprobs=True, top_logprobs=5, **base)
        plain = micro.generate(ids, seqs, **base)
        assert torch.equal(o.sequences, plain), tag
        cnt = o.n_tokens.cpu()
        assert len(set(cnt.tolist())) > 1, (tag, cnt)
        r = tlc.consistency(o, 5, True)
        _check_self(tag, r, True, greedy_plain=True)
        pos = torch.arange(o.sequences.shape[1])[None, :]
        tid = o.top_ids.cpu()
        assert bool((tid[pos >= cnt[:, None]] == -1).all()) and bool((tid[pos < cnt[:, None]] >= 0).all()), tag
    micro.set_stop_sequence(None)


def test_llama8b_width_batch64(big):
    ids, mask, seqs = gsc.batch(big.cfg, 64)
    res = {}
    for name, samp in (("greedy", None), ("sampled", SAMPLING)):
        res[name] = tlc.consistency(tlc.gen(big, ids, mask, seqs, 8, k=5, sampling=samp), 5, True)
        _check_self(name, res[name], True, greedy_plain=samp is None)
    record("top_logprobs.llama8b_b64", res)


def _forward_inputs(micro, k):
    """The micro prompts with their greedy answers as labels -> (generate()'s output, its counts, forward()'s arguments)."""
    g, ids, mask, seqs = _micro_inputs()
    pad, N, k = int(g["pad"]), 10, 5
    o = micro.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, eos_token_id=[int(g["eos"])],
                       return_dict_in_generate=True, output_token_logprobs=True, top_logprobs=k)
    gen, cnt = o.sequences.cpu(), o.n_tokens.cpu()
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
    return o, cnt, dict(input_ids=fids, attention_mask=fmask, labels=flab, seq=seqs, top_logprobs=k), (fids, fmask, flab, seqs)


def test_forward_lean_path_identical(micro):
    """forward(labels, top_logprobs=5, return_logits=False) gives the result of return_logits=True, bit for bit: with top log-probs
    on, the loss-only call runs the lm_head on the same rows through the same launches (the loss-only lm_head proper runs at
    another row count through other GEMM kernels, whose 16-bit logits differ in the last bit: 7.9e-3 on these inputs)."""
    k = 5
    _, _, kw, _ = _forward_inputs(micro, k)
    out = micro.forward(**kw)
    lean = micro.forward(return_logits=False, **kw)
    d = float((out.top_logprobs - lean.top_logprobs).abs().max())
    n_ids = int((out.top_ids != lean.top_ids).sum())
    print(f"forward paths: id mismatches {n_ids}, max |top_logprobs difference| {d:.3e}")
    record("top_logprobs.forward_paths", dict(id_mismatches=n_ids, lp_abs=d))
    assert torch.equal(out.top_ids, lean.top_ids) and torch.equal(out.top_logprobs, lean.top_logprobs), (n_ids, d)
    assert lean.logits is None and torch.equal(out.token_logprobs, lean.token_logprobs)


def test_forward_labels(micro):
    """forward(labels, top_logprobs=5): consistent with out.logits (16-bit values, stable order) and with token_logprobs on
    both paths, and at the generated positions consistent with generate()'s lists."""
    k = 5
    o, cnt, kw, (fids, fmask, flab, seqs) = _forward_inputs(micro, k)
    out = micro.forward(**kw)
    lean = micro.forward(return_logits=False, **kw)
    assert lean.logits is None and lean.top_ids.shape == out.top_ids.shape
    _, _, _, _, _, lab_out = micro.prepare_inputs_labels_for_multimodal(fids, None, fmask, None, flab, seqs)
    lab_out = lab_out.cpu()
    B, T = lab_out.shape
    assert out.top_ids.shape == out.top_logprobs.shape == (B, T, k) and out.top_ids.dtype == torch.int64
    tid, tlp, tok = out.top_ids.cpu().numpy(), out.top_logprobs.cpu().numpy(), out.token_logprobs.cpu().numpy()
    logits = out.logits.float().cpu().numpy()
    counted = (lab_out != -100).numpy()
    counted[:, 0] = False                                      # (no position predicts labels[:, 0])
    assert (tid[~counted] == -1).all() and (tlp[~counted] == 0).all()
    l_tid, l_tlp, l_tok = lean.top_ids.cpu().numpy(), lean.top_logprobs.cpu().numpy(), lean.token_logprobs.cpu().numpy()
    assert (l_tid[~counted] == -1).all() and (l_tlp[~counted] == 0).all() and (l_tid[counted] >= 0).all()
    assert np.array_equal(l_tlp, tlp) and np.array_equal(l_tid, tid)
    worst = vs_gen = 0.0
    shared = 0
    gid, glp = o.top_ids.cpu().numpy(), o.top_logprobs.cpu().numpy()
    for b in range(B):
        ts = np.flatnonzero(counted[b])
        assert ts.size == int(cnt[b])
        r_ids, r_lp, _ = tref.top_logprobs_ref(logits[b, ts - 1], k)            # position t - 1 predicts labels[b, t]
        assert np.array_equal(tid[b, ts], r_ids), b
        worst = max(worst, float(np.abs(tlp[b, ts] - r_lp).max()))
        for j, t in enumerate(ts):
            hit = np.flatnonzero(tid[b, t] == int(lab_out[b, t]))
            if hit.size:
                worst = max(worst, abs(float(tlp[b, t, hit[0]]) - float(tok[b, t])))
            hit = np.flatnonzero(l_tid[b, t] == int(lab_out[b, t]))               # the loss-only path against its own token_logprobs
            if hit.size:
                worst = max(worst, abs(float(l_tlp[b, t, hit[0]]) - float(l_tok[b, t])))
            for a, i in enumerate(gid[b, j]):                                     # the ids both lists share
                h = np.flatnonzero(tid[b, t] == i)
                if h.size:
                    shared += 1
                    vs_gen = max(vs_gen, abs(float(glp[b, j, a]) - float(tlp[b, t, h[0]])))
    record("top_logprobs.forward", dict(vs_logits_abs=worst, vs_generate_abs=vs_gen, shared=shared))
    assert worst < SELF_ABS and shared > 0 and vs_gen < DECODE_VS_PREFILL, (worst, vs_gen, shared)


def test_eval_loop_save_top_logprobs():
    """eval_ddp.annotate(top_logprobs_out=..., top_k=K) (--save_top_logprobs): the same ids as without it, and per item the K
    alternatives of every counted step, the chosen id's log-prob among them where it is one of them."""
    import importlib.util
    from opus_pllm_amd import builder, synth
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=258, max_prompt=64, max_new_tokens=8)
    items = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(20 + 11 * (i % 9), i), output="x")
             for i in range(7)]
    plain = ddp.annotate(model, tok, items, "", 4, 8, temperature=0.0, top_p=0.95)
    lps, tops = [], []
    with_top = ddp.annotate(model, tok, items, "", 4, 8, temperature=0.0, top_p=0.95, logprobs_out=lps, top_logprobs_out=tops, top_k=3)
    assert torch.equal(plain, with_top)
    with_top = with_top.cpu()
    tid = torch.cat([x[0] for x in tops]).cpu()
    tlp = torch.cat([x[1] for x in tops]).cpu()
    lp, n = torch.cat([x[0] for x in lps]).cpu(), torch.cat([x[1] for x in lps]).cpu()
    assert tid.shape == tlp.shape == (7, 8, 3)
    pos = torch.arange(8)[None, :]
    assert bool((tid[pos >= n[:, None]] == -1).all()) and bool((tid[pos < n[:, None]] >= 0).all())
    assert bool((tid[:, :, 0] == with_top)[pos < n[:, None]].all()) and bool((tlp[:, :, 0] == lp)[pos < n[:, None]].all())


def test_bf16_build_top_logprobs():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_top_logprobs_check.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_TOP_LOGPROBS ")][-1]
    o = json.loads(line[len("BF16_TOP_LOGPROBS "):])
    record("top_logprobs.bf16", o)
    assert o["operand_dtype"] == 1, o
    for name, res in o["kernel"].items():
        _check_kernel(res)
    for name, r in o["self"].items():
        _check_self(name, r, True, greedy_plain=name == "greedy")
