"""Prompt-lookup decoding on the GPU (generate(prompt_lookup_num_tokens=k), opus_llama_verify_step, csrc/lookup.hip): the draft
and commit kernels against the twin (tests/lookup_ref.py) bit for bit, the verify pass against prefill of the extended prompt
under the project's "decode step against prefill of the longer prompt" bounds (2e-3 rel-L2 at Llama-3-8B widths, 1.5e-2 on the
micro fixtures; the bf16 row: 1.5e-2 / 2e-2), stale cache slots, and generate() end to end against the goldens."""
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from gpu_helpers import record
import lookup_checks as LC
import lookup_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE_BOUND = 2e-3           # tests/test_gpu_batch64.py: decode step vs prefill of the longer prompt, Llama-3-8B widths
MICRO_BOUND = 1.5e-2        # tests/test_gpu_parity.py REL_L2
K_REL = 2e-3                # tests/attn_decode_checks.py: the appended key within 2e-3 max |ref|
TPS = (30, 31, 62, 63, 64)  # the appended positions straddle the 32- and 64-slot tile borders of the attention kernels
PADS = (0, 7, 33)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def micro64(dev):
    model = LC.make_model(opa.micro(max_batch=64, max_prompt=96, max_new_tokens=24), dev)
    yield model
    del model


@pytest.fixture(scope="module")
def wide(dev):
    model = LC.make_model(LC.wide_cfg(64), dev)
    yield model
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the draft kernel
@pytest.mark.parametrize("R", [1, 3, 64])
def test_draft_kernel_equals_the_twin(micro64, dev, R):
    lib, ctx = micro64._lib, micro64._ctx
    for L in (1, 2, 255, 256, 257, 601):
        rows = LC.draft_histories(R, L, 4 + (L % 3), seed=L + R)
        for m in (1, 2, 3):
            for k in (1, 7, 15):
                bad = LC.draft_mismatches(lib, ctx, dev, rows, k, m)
                assert not bad, (R, L, m, k, bad[:2])
    # ragged lengths in one launch, and histories that match only late (starts past the first 256: several starts per thread)
    rows = [[9] * 300 + [1, 2, 3, 4, 1, 2], [7] * 599 + [5, 7], list(range(20, 620)) + [25]][: max(1, min(R, 3))]
    for m in (1, 2, 3):
        assert not LC.draft_mismatches(lib, ctx, dev, rows, 7, m)


def test_draft_kernel_sentinel_cases(micro64, dev):
    rows = LC.sentinel_histories()
    for m in (1, 2, 3):
        for k in (1, 7, 15):
            assert not LC.draft_mismatches(micro64._lib, micro64._ctx, dev, rows, k, m), (m, k)
    got, got_len = LC.run_draft(micro64._lib, micro64._ctx, dev, rows, 7, 2)
    assert got_len == [0, 2, 0, 1, 2, 0] and got[1][:2] == [3, 9] and got[3][0] == 9


# ------------------------------------------------------------------------------------------------ the commit kernel
def test_commit_kernel_equals_the_twin(micro64, dev, gold):
    for name, st, x, y, dl, eos, stop in LC.commit_cases(gold("generate_micro")["free_ids"]):
        ids, fin, step, nxt, nunf, words = LC.run_accept(micro64._lib, micro64._ctx, dev, st, x, y, dl, 1, eos, stop)
        a, unf, drafted = LR.commit(st, x, y, dl, 1, eos, stop)            # (advances the twin's state in place)
        assert (ids, fin, step, nxt, nunf) == (st.ids, st.fin, st.step, st.next, st.n_unf), name
        assert words == [a, unf, st.step, drafted], name
    # behind a plain step (pre = 0): one position, committed at the step word's column
    st = LR.State(3, 12, 2)
    st.step = 4
    y = [[11], [85], [13]]
    got = LC.run_accept(micro64._lib, micro64._ctx, dev, st, [[2]] * 3, y, [0, 0, 0], 0, (85,), ())
    LR.commit(st, [[2]] * 3, y, [0, 0, 0], 0, (85,), ())
    assert got[:5] == (st.ids, st.fin, st.step, st.next, st.n_unf) and st.step == 4 and st.fin == [0, 1, 0]


# ------------------------------------------------------------------------------------------------ verify_step against prefill
def _verify_cases(R):
    for i, Tp in enumerate(TPS):
        if R == 1:
            for p in PADS:
                if p < Tp - 2:                                       # (a row needs real tokens in front of the pass)
                    yield Tp, [p]
        else:
            pads = [PADS[(i + r) % 3] for r in range(R)]
            yield Tp, [p if p < Tp - 2 else 7 for p in pads]


@pytest.mark.parametrize("n", [1, 2, 8, 16])
@pytest.mark.parametrize("R", [1, 3])
def test_verify_step_logits_micro(micro64, R, n):
    worst = 0.0
    for Tp, pads in _verify_cases(R):
        o = LC.verify_vs_prefill(micro64, R, Tp, pads, n, seed=Tp + n)
        print("verify micro", R, n, Tp, pads, o)
        worst = max(worst, o["rel_l2"])
        assert o["rel_l2"] < MICRO_BOUND and o["argmax_equal"], (R, n, Tp, pads, o)
    record(f"lookup.verify_vs_prefill.micro.R{R}.n{n}", worst)


@pytest.mark.parametrize("n", [1, 2, 8, 16])
@pytest.mark.parametrize("R", [1, 3])
def test_verify_step_logits_llama3_8b_widths(wide, R, n):
    worst = 0.0
    for Tp, pads in _verify_cases(R):
        o = LC.verify_vs_prefill(wide, R, Tp, pads, n, seed=Tp + n)
        print("verify wide", R, n, Tp, pads, o)
        worst = max(worst, o["rel_l2"])
        assert o["rel_l2"] < WIDE_BOUND and o["argmax_equal"], (R, n, Tp, pads, o)
    record(f"lookup.verify_vs_prefill.wide.R{R}.n{n}", worst)


@pytest.mark.parametrize("which", ["micro", "wide"])
def test_verify_step_fills_max_batch(micro64, wide, which):
    """R n = 64 logits rows at max_batch 64; one more row is refused with OPUS_ESHAPE."""
    model, bound = (micro64, MICRO_BOUND) if which == "micro" else (wide, WIDE_BOUND)
    o = LC.verify_vs_prefill(model, 4, 64, [0, 7, 33, 1], 16, seed=11)
    print("verify R n = 64", which, o)
    assert o["rel_l2"] < bound and o["argmax_equal"], o
    ids, mask = LC.random_prompt(model.cfg, 5, 30, [0] * 5, 1)
    model.prefill_logits(LC.embed(model, ids), mask)
    with pytest.raises(_cabi.OpusError) as e:
        model.verify_step(torch.ones((5, 13), dtype=torch.int32))
    assert e.value.code == -2 and "max_batch" in str(e.value)


@pytest.mark.parametrize("which", ["micro", "wide"])
def test_verify_step_appends_keys_and_values(micro64, wide, which):
    """The decode attention's rule for what a step appends (tests/attn_decode_checks.py: the key within 2e-3 max |ref|, the value
    bit-exact, both against the step's OWN projections) on the last layer, whose projections the context still holds: here both
    are bit-exact.  Against the prefill of the extended prompt, every layer: keys within 2e-3 max |ref| (observed <= 9.3e-4);
    the values are within 7.0e-4 of max |ref| there but NOT bit-equal - the prefill projects its rows through other GEMM kernels,
    and from layer 1 on from an attention output that differs in the last bits - so bit-equality to the prefill is recorded
    (`value_bit_equal_to_prefill`), not asserted."""
    model = micro64 if which == "micro" else wide
    for R, Tp, pads, n in ((3, 62, [0, 7, 33], 8), (3, 31, [7, 0, 3], 2), (1, 63, [33], 16)):
        o = LC.verify_kv(model, R, Tp, pads, n, seed=Tp)
        print("verify kv", which, R, Tp, n, o)
        record(f"lookup.verify_kv.{which}.R{R}.Tp{Tp}.n{n}", o)
        assert o["last_layer_key_exact"] and o["last_layer_value_exact"] and o["prompt_slots_untouched"], o
        assert o["key_err"] <= K_REL and o["value_err"] <= K_REL, o


def test_stale_slots_are_never_read(micro64, wide):
    """lookup_checks.stale_slots: behind a pass that rejected six positions, the next pass and a plain decode step are bit-identical
    whatever the rejected positions left in the cache (states A and A').  Against state B (a first pass of n = 2: no stale
    slot) the results are NOT bit-identical and cannot be: B's accepted positions ran in launches of another shape (observed
    rel-L2 between A and B on the MI355X: see profiles/lookup_parity.jsonl), so that comparison is held to the bound of two launch
    shapes of one computation instead."""
    for model, bound, tag in ((micro64, MICRO_BOUND, "micro"), (wide, WIDE_BOUND, "wide")):
        o = LC.stale_slots(model)
        print("stale slots", tag, o)
        record(f"lookup.stale_slots.{tag}", o)
        assert o["second_pass_identical"] and o["plain_step_identical"] and o["a2"] == [0, 0, 0], o
        assert o["b_second_pass_rel_l2"] < bound and o["b_plain_step_rel_l2"] < bound, o


# ------------------------------------------------------------------------------------------------ end to end
def _gold_inputs(gold, gold_dir, name="generate_micro"):
    g = gold(name)
    seqs = json.load(open(os.path.join(gold_dir, name + ".seqs.json")))
    return g, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), seqs


@pytest.mark.parametrize("preset,tag", [("micro", "generate_micro"), ("micro_qwen", "generate_micro_qwen"),
                                        ("micro_opt", "generate_micro_opt")])
def test_generate_equals_the_goldens(dev, gold, gold_dir, preset, tag):
    g, ids, mask, seqs = _gold_inputs(gold, gold_dir)
    gq = gold(tag)
    seed = int(gq["weights_seed"]) if "weights_seed" in gq.files else 0
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    cfg = opa.PRESETS[preset](max_batch=24)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, seed), dev), dev)
    free = torch.from_numpy(gq["free_ids"])
    kw = dict(attention_mask=mask, pad_token_id=int(g["pad"]), do_sample=False, max_new_tokens=free.shape[1])
    if tag == "generate_micro":
        out = model.generate(ids, seqs, prompt_lookup_num_tokens=7, **kw).cpu()
        assert torch.equal(out, free)
        out = model.generate(ids, seqs, prompt_lookup_num_tokens=7, eos_token_id=[int(g["eos"])], **kw).cpu()
        assert torch.equal(out, torch.from_numpy(g["eos_ids_out"]))                     # EOS-then-pad row
    else:                                                     # (the family goldens are on the spliced embeddings of generate_micro)
        emb, mo = torch.from_numpy(g["embeds"]).to(dev, _cabi.operand_dtype()), torch.from_numpy(g["mask_out"]).to(dev)
        hist = ([[1, 2]] * 3, [2, 2, 2])
        import numpy as np
        out, stats = model._lookup(emb, mo, free.shape[1], [], 2, 7, 2, (np.asarray(hist[0], dtype=np.int32), np.asarray(hist[1])))
        assert torch.equal(out.cpu(), free)
        assert torch.equal(model._greedy(emb, mo, free.shape[1], [], 2).cpu(), free)
    # the golden answer as the corpus: the same ids in fewer passes; a corpus of ids the model never emits: the same ids, nothing accepted
    if tag == "generate_micro":
        res = model.generate(ids, seqs, prompt_lookup_num_tokens=7, lookup_ids=free, return_dict_in_generate=True, **kw)
        assert torch.equal(res.sequences.cpu(), free)
        st = res.stats
        print("lookup stats (golden corpus)", st)
        assert st.accepted > 0 and st.passes + st.plain_steps < free.shape[1]
        never = sorted(set(range(3, cfg.dec_vocab)) - set(free.flatten().tolist()) - set(ids.flatten().tolist()))[:9]
        res = model.generate(ids, seqs, prompt_lookup_num_tokens=7, lookup_ids=[never] * 3, return_dict_in_generate=True, **kw)
        assert torch.equal(res.sequences.cpu(), free) and res.stats.accepted == 0
        # plain generate() afterwards is what it was (the captured step is untouched by the lookup call)
        assert torch.equal(model.generate(ids, seqs, **kw).cpu(), free)


@pytest.fixture(scope="module")
def micro_long(dev, gold):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    g = gold("generate_micro_long")
    cfg = opa.micro(max_prompt=80, max_new_tokens=288, max_batch=24)
    canon = synth.canonical_weights(cfg, int(g["weights_seed"]))
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, canon, dev), dev)
    yield cfg, model, g
    del model


def test_generate_micro_long_margins_then_ids(micro_long, gold_dir):
    """The 816 ids of generate_micro_long under that fixture's rule (tests/test_gpu_longctx.py): first the error of the DIFFERENCE
    of the two leading logits, teacher-forced through verify_step in passes of 8, stays below 0.75 x the smallest reference margin
    (0.0247); then generate(prompt_lookup_num_tokens=7) gives the reference's ids."""
    cfg, model, g = micro_long
    seqs = json.load(open(os.path.join(gold_dir, "generate_micro_long.seqs.json")))
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    ref, ref_margin = torch.from_numpy(g["free_ids"]), torch.from_numpy(g["margins"])
    prot = model.switch_projector_embedding(model.encode_projector_embedding(model.encode_seq2embedding(seqs)))
    emb, mo, _ = model._splice(ids, mask, prot, True)
    lg = model.prefill_logits(emb, mo).cpu()
    assert torch.equal(lg.argmax(-1), ref[:, 0])
    top2 = lg.topk(2, dim=-1).values
    worst = float(((top2[:, 0] - top2[:, 1]) - ref_margin[:, 0]).abs().max())
    N, s_ = ref.shape[1], 0
    while s_ + 1 < N:                                          # ids s_ .. s_ + n - 1 are fed, predicting ids s_ + 1 .. s_ + n
        n = min(8, N - 1 - s_)
        lg, arg, a = model.verify_step(ref[:, s_:s_ + n])
        assert a == n - 1 and torch.equal(arg.cpu().long(), ref[:, s_ + 1:s_ + 1 + n]), s_
        top2 = lg.cpu().topk(2, dim=-1).values
        worst = max(worst, float(((top2[..., 0] - top2[..., 1]) - ref_margin[:, s_ + 1:s_ + 1 + n]).abs().max()))
        s_ += n
    record("lookup.generate_micro_long.margin_max_abs_err", worst)
    print("generate_micro_long margin error through verify_step", worst, "bound", 0.75 * float(g["min_margin"]))
    assert worst < 0.75 * float(g["min_margin"]), worst
    res = model.generate(ids, seqs, attention_mask=mask, pad_token_id=int(g["pad"]), do_sample=False, max_new_tokens=N,
                         prompt_lookup_num_tokens=7, return_dict_in_generate=True)
    record("lookup.generate_micro_long.stats", repr(res.stats))
    assert torch.equal(res.sequences.cpu(), ref)
    assert res.stats.passes + res.stats.plain_steps <= N - 1


def test_generate_batch3_ragged_and_stop_sequence(dev, gold, gold_dir):
    """Three rows left-padded by 2, 0 and 7 (the generate_micro fixture: every id is decided by a margin of 0.10 or more, so the
    pass's kernels and the decode step's agree on it)."""
    g, ids, mask, seqs = _gold_inputs(gold, gold_dir)
    model = LC.make_model(opa.micro(max_batch=24), dev)
    N = g["free_ids"].shape[1]
    plain, got, stats = LC.e2e(model, ids, mask, seqs, N, k=7)
    assert torch.equal(plain, torch.from_numpy(g["free_ids"])) and torch.equal(plain, got), stats
    plain, got, stats = LC.e2e(model, ids, mask, seqs, N, k=7, lookup_ids=plain)
    assert torch.equal(plain, got) and stats.accepted > 0 and stats.passes + stats.plain_steps < N, stats
    # EOS and the stop sequence taken from the plain answer: rows end at different columns, inside accepted chains
    eos = [int(g["eos"])]
    stop = [int(plain[0, 7]), int(plain[0, 8])]
    for corpus in (None, plain):
        kw = {} if corpus is None else {"lookup_ids": corpus}
        p2, g2, st2 = LC.e2e(model, ids, mask, seqs, N, k=7, eos_token_id=eos, stop_sequence=stop, **kw)
        assert torch.equal(p2, g2), (st2, p2, g2)
    model.set_stop_sequence(None)
    # k = 1 and a budget of one and two ids
    for mx in (1, 2, 5):
        p3, g3, _ = LC.e2e(model, ids, mask, seqs, mx, k=1, lookup_ids=plain)
        assert torch.equal(p3, g3), mx
    # batch 1: transformers' algorithm
    p4, g4, st4 = LC.e2e(model, ids[1:2], mask[1:2], seqs[1:2], N, k=7, lookup_ids=plain[1:2])
    assert torch.equal(p4, g4) and st4.accepted > 0


# ------------------------------------------------------------------------------------------------ FP8
def test_fp8_verify_step_is_the_dequantised_twins(dev):
    cfg = LC.wide_cfg(16)
    m8 = LC.make_model(cfg, dev, decoder_weights="fp8")
    m16 = LC.make_model(cfg, dev, decoder_weights="fp8_dequantized")
    for R, n in ((1, 8), (3, 5)):
        ids, mask = LC.random_prompt(cfg, R, 31, [0, 7, 3][:R], 5)
        toks = torch.randint(3, cfg.dec_vocab, (R, n), generator=torch.Generator().manual_seed(6))
        outs = []
        for m in (m8, m16):
            m.prefill_logits(LC.embed(m, ids), mask)
            before = m.stat("w8_gemms")
            lg, arg, a = m.verify_step(toks)
            outs.append((lg.cpu(), m.stat("w8_gemms") - before))
        assert torch.equal(outs[0][0], outs[1][0]), (R, n)
        print("fp8 verify_step w8_gemms", R, n, outs[0][1])
        assert outs[0][1] > 0 and outs[1][1] == 0, (R, n, outs[0][1], outs[1][1])
    # a whole lookup call: the FP8 model's ids are its twin's (the logits are, bit for bit), and its FP8 GEMM count rises
    ids, mask, seqs = LC.ragged_inputs(cfg, 2)
    kw = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=8, prompt_lookup_num_tokens=7)
    first = m16.generate(ids, seqs, **kw)
    kw["lookup_ids"] = first                                   # (so that drafts are verified: passes, not only plain steps)
    before, passes = m8.stat("w8_gemms"), m8.stat("lookup_passes")
    assert torch.equal(m8.generate(ids, seqs, **kw), m16.generate(ids, seqs, **kw))
    assert m8.stat("w8_gemms") > before and m8.stat("lookup_passes") > passes
    del m8, m16
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the bf16 build
def test_bf16_build_lookup():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_lookup_check.py")], capture_output=True, text=True,
                       env=dict(os.environ, OPUS_DTYPE="bf16"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_LOOKUP ")][-1]
    o = json.loads(line[len("BF16_LOOKUP "):])
    record("lookup.bf16", o)
    assert o["operand_dtype"] == 1 and o["draft_mismatches"] == 0
    # the bf16 row of "decode step against prefill of the longer prompt" (tests/test_gpu_bf16.py): 1.5e-2 at full widths, 2e-2 micro
    assert o["wide_rel_l2"] < 1.5e-2 and o["micro_rel_l2"] < 2e-2, o
    assert o["stale"]["second_pass_identical"] and o["stale"]["plain_step_identical"], o
    assert o["kv"]["last_layer_key_exact"] and o["kv"]["last_layer_value_exact"] and o["kv"]["prompt_slots_untouched"], o
    assert o["kv"]["key_err"] <= 8 * K_REL, o                   # bf16: 8 significand bits against fp16's 11
    assert o["e2e_equal"] and o["e2e_accepted"] > 0, o
